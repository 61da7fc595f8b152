"""GPU tests of Track X's Adam and AdamW (include/rcn_hipx.h, rcn_hipx_set_adam; csrc/convnet_adam.hpp): the update inside the step's
reduction launch in all eight forms, the tick on the device inside the captured graph, the data-parallel half, the state entries, and that
a net without Adam is untouched.

The twin-net method of tests/test_gpu_convnet_update_forms.py: net A steps, net B supplies the gradient at A's parameters, and
tests/_adam_ref.py updates on the host in float32; the assertions are on bits.  There is no comparison of Adam's parameters with the f64
oracle: its early updates are about +-lr whatever the gradient's size, so fp32 gradient noise on near-zero elements is amplified to lr and no
honest tolerance exists.  The chain is closed by GPU == float32 restatement (bits, here) and restatement == torch (float64,
tests/test_convnet_adam.py)."""
import itertools

import numpy as np
import pytest
from _accum_ref import accumulate
from _adam_ref import TICK0, adam_tick, adam_ticks, adam_update
from _clip_ref import apply_coef, grad_norm
from _convnet_util import (FUSED_HEAD, NESTEROV, PLAIN, PLAIN_HEAD, POOL_PAIRS, batch, batches, check_norm, grad, make_net, oracle_params, same_bits,
                           same_state, step, twins, zeros)
from _ema_ref import ema_update

pytestmark = pytest.mark.gpu

DECAY = 0.9
LRS = [0.05, 0.05, 0.02, 0.05]                          # eager, replay, a second rate (a second graph), back to the first
ADAM = dict(betas=(0.9, 0.999), eps=1e-8, weight_decay=5e-4, decoupled=False)
ADAMW = dict(betas=(0.9, 0.999), eps=1e-8, weight_decay=5e-2, decoupled=True)
KINDS = {"adam": ADAM, "adamw": ADAMW}


class Host:
    """the float32 restatement's state beside a net: parameters, moments and the tick"""

    def __init__(self, p, cfg, m=None, v=None, tick=TICK0):
        self.p, self.cfg, self.tick = p.copy(), dict(cfg), tick
        self.m = np.zeros_like(p) if m is None else m.copy()
        self.v = np.zeros_like(p) if v is None else v.copy()

    def update(self, g, lr):
        c = self.cfg
        self.tick, c1, c2 = adam_tick(self.tick, *c["betas"])
        self.p, self.m, self.v = adam_update(self.p, g, self.m, self.v, lr, c1, c2, c["betas"][0], c["betas"][1], c["eps"], c["weight_decay"], c["decoupled"])

    def check(self, net, tag):
        m, v, count = net.get_adam_state()
        p = net.get_params()
        assert same_bits(p, self.p), (tag, "p", float(np.abs(p - self.p).max()))
        assert same_bits(m, self.m), (tag, "m", float(np.abs(m - self.m).max()))
        assert same_bits(v, self.v), (tag, "v", float(np.abs(v - self.v).max()))
        assert count == self.tick[0], (tag, count, self.tick[0])


def same_adam(a, b):
    (ma, va, sa), (mb, vb, sb) = a.get_adam_state(), b.get_adam_state()
    return same_bits(a.get_params(), b.get_params()) and same_bits(ma, mb) and same_bits(va, vb) and sa == sb


FORMS = list(itertools.product(["adam", "adamw"], [False, True], [False, True], [1, 2]))      # (kind, clip, ema, accumulate)
FORM_IDS = [kind + ("-clip" if c else "-noclip") + ("-ema" if e else "-noema") + f"-acc{k}" for kind, c, e, k in FORMS]


@pytest.mark.parametrize("kind,clip,ema,k", FORMS, ids=FORM_IDS)
def test_train_step_is_the_host_update_bit_for_bit(kind, clip, ema, k):
    """four updates (of k micro-batches each, every one with its own data) against the NumPy restatements: the rate from the host"""
    spec, cfg = PLAIN_HEAD, KINDS[kind]
    a, b = twins(spec, "fp32")
    a.set_adam(**cfg)
    if ema:
        a.set_ema(DECAY)
    if k > 1:
        a.set_accumulate(k)
    plan = a.plan_of_this_net(spec[2])
    assert "  tick: k_adam_tick, 1 thread (update count and bias corrections on the device)\n  update: k_reduce_all_adam" in plan, plan
    assert f"(Adam: betas 0.9 0.999, eps 1e-08, weight decay {cfg['weight_decay']:g}, {'decoupled' if cfg['decoupled'] else 'L2'})" in plan, plan
    data = [batch(a, spec, 20 + j) for j in range(k)]
    h = Host(a.get_params(), cfg)
    e = h.p.copy()
    max_norm = None
    if clip:
        first = [grad(b, x, y, h.p)[1] for x, y in data]
        max_norm = float(grad_norm(accumulate(first, k) if k > 1 else first[0]) / np.float32(2))       # half the first update's norm
        a.set_clip(max_norm)
        assert "k_reduce_all_clip_adam" in a.plan_of_this_net(spec[2])
    for u, lr in enumerate(LRS):
        logical, padded = [], []
        for j, (x, y) in enumerate(data):
            gdev, gpad = grad(b, x, y, h.p)
            logical.append(b.unpad(gdev))
            padded.append(gpad)
            step(a, x, y, lr)
            if k > 1:
                assert same_bits(a.get_accumulated(), accumulate(logical, k)), (u, j)
            if j < k - 1:                                # a first or middle micro-step: no update, no tick
                h.check(a, (u, j))
        g, gpad = (accumulate(logical, k), accumulate(padded, k)) if k > 1 else (logical[0], padded[0])
        if clip:
            norm, coef = a.grad_norm()
            check_norm(f"update {u}", norm, coef, grad_norm(gpad), max_norm)
            assert u > 0 or coef < 1.0
            g = apply_coef(g, coef)
        h.update(g, lr)
        if ema:
            e = ema_update(e, h.p, DECAY)
        h.check(a, u)
        if ema:
            assert same_bits(a.get_ema(), e), u
    assert a.get_adam_state()[2] == len(LRS)
    if clip:
        assert a.grad_norm_count() == len(LRS)
    a.close(); b.close()


@pytest.mark.parametrize("precision", ["fp32", "bf16_stored"])
def test_many_chunk_job_under_the_adam_functor(precision):
    """POOL_PAIRS: the first layer's job has 16 chunks -- the GR > 1 and i < jb.n edges of reduce_all_body under AdamUpdate; three steps"""
    spec = POOL_PAIRS
    a, b = twins(spec, precision)
    a.set_adam(**ADAM)
    x, y = batches(a, spec, 1)[0]
    h = Host(a.get_params(), ADAM)
    for u, lr in enumerate([0.01, 0.01, 0.004]):
        g = b.unpad(grad(b, x, y, h.p)[0])
        step(a, x, y, lr)
        h.update(g, lr)
        h.check(a, u)
    assert np.abs(h.v).max() > 0
    a.close(); b.close()


@pytest.mark.parametrize("clip,ema", list(itertools.product([False, True], [False, True])), ids=["noclip-noema", "noclip-ema", "clip-noema", "clip-ema"])
def test_epoch_with_device_rate_is_the_batches_fed_one_by_one(clip, ema):
    """train_epoch over a resident uint8 set of four batches, the rate from a device tensor (the _dlr forms), against a twin fed the same
    batches by gather_batch + train_step at the same float rates; one graph for the epoch, none for the second, eight ticks"""
    import torch
    spec = PLAIN_HEAD
    in_shape, layers, B = spec
    a, t = twins(spec, "fp32")
    rng = np.random.default_rng(6)
    X = a.to_device(rng.integers(0, 256, (4 * B,) + in_shape).astype(np.uint8))
    Y = a.to_device(rng.integers(0, layers[-1][1], 4 * B).astype(np.int32))
    rates = np.array([0.01, 0.05, 0.03, 0.02], dtype=np.float32)
    lr = a.to_device(rates)
    a.synchronize()
    if clip:
        with torch.cuda.stream(t.stream):
            x0, y0 = t.gather_batch(X, Y, None, B)
        max_norm = float(grad_norm(grad(t, x0, y0)[1]) / np.float32(4))
    for n in (a, t):
        n.set_adam(**ADAM)
        if ema:
            n.set_ema(DECAY)
        if clip:
            n.set_clip(max_norm)
    plan = a.plan_epoch_of_this_net(B, lr_from_device=True)
    assert "k_adam_tick" in plan and "k_reduce_all" + ("_clip" if clip else "") + "_adam" + ("_ema" if ema else "") + "_dlr" in plan, plan
    g0 = a.graphs_instantiated()
    keep = []
    for ep in range(2):
        with torch.cuda.stream(a.stream):
            a.train_epoch(X, Y, None, B, lr)
        a.synchronize()
        assert a.graphs_instantiated() == g0 + 1, ep     # one graph per B whatever the rate; the second epoch adds none
        for s in range(4):
            with torch.cuda.stream(t.stream):
                x, y = t.gather_batch(X, Y, None, B, base=s * B)
                keep.append((x, y))
                t.train_step(x, y, float(rates[s]))
            t.synchronize()
            if clip and ep == 0 and s == 0:
                assert t.grad_norm()[1] < 1.0            # clipping bites on the first update
        assert same_adam(a, t), ep
        if ema:
            assert same_bits(a.get_ema(), t.get_ema()), ep
        if clip:
            assert a.grad_norm() == t.grad_norm()
    assert a.get_adam_state()[2] == 8
    a.close(); t.close()


@pytest.mark.parametrize("clip", [False, True], ids=["noclip", "clip"])
def test_data_parallel_half_is_the_fused_step_bit_for_bit(clip):
    """gradients_bucketed + apply_sgd(grad, 1, lr) == train_step over three steps: parameters, moments and count; apply_sgd(2 g, 0.5, lr)
    too.  rcn_hipx_apply_dev stays the plain axpy and leaves m, v and the count alone."""
    import torch
    spec = POOL_PAIRS
    a, b, c = twins(spec, "fp32", count=3)
    x, y = batches(a, spec, 1)[0]
    max_norm = float(grad_norm(grad(b, x, y)[1]) / np.float32(2)) if clip else None
    for n in (a, b, c):
        n.set_adam(**ADAM)
        if clip:
            n.set_clip(max_norm)
    g = torch.empty(b.n_padded, dtype=torch.float32, device=b.device)
    lr = 0.003
    for u in range(3):
        step(a, x, y, lr)
        with torch.cuda.stream(b.stream):
            b.gradients_bucketed(x, y, g, None, 0)
            b.apply_sgd(g, 1.0, lr)
        b.synchronize()
        with torch.cuda.stream(c.stream):
            c.gradients_bucketed(x, y, g, None, 64 << 10)
            g2 = g * 2.0
            c.apply_sgd(g2, 0.5, lr)
        c.synchronize()
        for n in (b, c):
            assert same_adam(n, a), u
            if clip:
                assert n.grad_norm() == a.grad_norm(), u
        if clip and u == 0:
            assert a.grad_norm()[1] < 1.0
    assert a.get_adam_state()[2] == 3
    p_before, (m, v, count) = b.get_params(), b.get_adam_state()
    with torch.cuda.stream(b.stream):
        b.apply(g, lr)
    b.synchronize()
    m2, v2, count2 = b.get_adam_state()
    assert same_bits(m2, m) and same_bits(v2, v) and count2 == count == 3 and not same_bits(b.get_params(), p_before)
    a.close(); b.close(); c.close()


def test_state_saved_and_loaded_reset_switched_and_betas_changed():
    spec = FUSED_HEAD
    a, b = twins(spec, "fp32")
    a.set_adam(**ADAM)
    assert a.get_adam() == {"betas": (pytest.approx(0.9), pytest.approx(0.999)), "eps": pytest.approx(1e-8), "weight_decay": pytest.approx(5e-4),
                            "decoupled": False, "selected": True}
    three = batches(a, spec, 3, seed=4)
    lr = 0.01
    h = Host(a.get_params(), ADAM)
    for u in range(3):
        x, y = three[u]
        h.update(b.unpad(grad(b, x, y, h.p)[0]), lr)
        step(a, x, y, lr)
    h.check(a, "three steps")
    # a fresh net continues from the saved state
    m3, v3, count = a.get_adam_state()
    assert count == 3
    c = make_net(spec)
    c.set_params(a.get_params())
    c.set_adam(**ADAM)
    c.set_adam_state(m3, v3, 3)
    for u in range(2):
        step(a, *three[u], lr)
        step(c, *three[u], lr)
    assert same_adam(a, c) and a.get_adam_state()[2] == 5
    # the state survives set_params and a change of precision
    c.set_params(a.get_params())
    c.set_precision("bf16")
    c.set_precision("fp32")
    assert same_adam(a, c)
    # reset_adam
    c.reset_adam()
    m, v, count = c.get_adam_state()
    assert count == 0 and not m.any() and not v.any()
    c.close()

    # set_sgd, one step, set_adam again: Adam's state as it was, the velocity kept
    a.set_adam_state(m3, v3, 3)
    a.set_params(h.p)
    a.set_sgd(*NESTEROV)
    assert a.get_adam()["selected"] is False and "adam" not in a.plan_of_this_net(spec[2])
    step(a, *three[0], lr)
    vel = a.get_velocity()
    assert vel.any()
    a.set_adam(**ADAM)
    m, v, count = a.get_adam_state()
    assert same_bits(m, m3) and same_bits(v, v3) and count == 3 and same_bits(a.get_velocity(), vel) and a.get_adam()["selected"] is True

    # betas changed at step 3: the running products are rebuilt from the count, as if every tick had used the new betas
    changed = dict(ADAM, betas=(0.8, 0.99))
    a.set_adam(**changed)
    assert a.get_adam_state()[2] == 3
    h2 = Host(a.get_params(), changed, m3, v3, adam_ticks(3, 0.8, 0.99)[0])
    for u in range(2):                                   # eager, then a replay
        x, y = three[1]
        h2.update(b.unpad(grad(b, x, y, h2.p)[0]), lr)
        step(a, x, y, lr)
        h2.check(a, ("changed betas", u))
    assert h2.tick[0] == 5
    a.close(); b.close()


@pytest.mark.parametrize("sgd", [PLAIN, NESTEROV], ids=["plain", "nesterov"])
def test_nets_without_adam_are_untouched(sgd):
    """a net that had set_adam and then set_sgd back is a net that never had it: the same plan text, the same bits over four steps"""
    from mercer_research_amd.convnet import ConvNetError
    spec = FUSED_HEAD
    B = spec[2]
    a, b = twins(spec, "fp32", sgd=sgd)
    with pytest.raises(ConvNetError, match="status -6"):
        b.get_adam_state()
    with pytest.raises(ConvNetError, match="status -6"):
        b.set_adam_state(np.zeros(b.n_logical, dtype=np.float32), np.zeros(b.n_logical, dtype=np.float32), 0)
    b.reset_adam()                                       # (a no-op without state)
    assert b.get_adam()["selected"] is False
    a.set_adam(**ADAMW)
    assert "k_adam_tick" in a.plan_of_this_net(B)
    a.set_sgd(*sgd)                                      # unchanged values: it still selects SGD again
    assert a.get_adam()["selected"] is False and a.get_sgd() == b.get_sgd()
    for lr_dev in (False, True):
        assert a.plan_epoch_of_this_net(B, lr_from_device=lr_dev) == b.plan_epoch_of_this_net(B, lr_from_device=lr_dev)
    plan = a.plan_of_this_net(B)
    assert plan == b.plan_of_this_net(B) and "adam" not in plan.lower() and "tick" not in plan
    x, y = batches(a, spec, 1)[0]
    for lr in LRS:
        step(a, x, y, lr)
        step(b, x, y, lr)
        assert same_state(a, b)
    m, v, count = a.get_adam_state()
    assert count == 0 and not m.any() and not v.any()
    a.close(); b.close()


def test_invalid_settings_are_refused_and_change_nothing():
    from mercer_research_amd.convnet import ConvNetError
    nan, inf = float("nan"), float("inf")
    net = make_net(FUSED_HEAD)
    net.set_adam((0.8, 0.99), 1e-6, 1e-3, True)
    before = net.get_adam()
    assert before == {"betas": (pytest.approx(0.8), pytest.approx(0.99)), "eps": pytest.approx(1e-6), "weight_decay": pytest.approx(1e-3), "decoupled": True,
                      "selected": True}
    bad = [dict(betas=(1.0, 0.999)), dict(betas=(-0.1, 0.999)), dict(betas=(nan, 0.999)), dict(betas=(inf, 0.999)), dict(betas=(0.9, 1.0)),
           dict(betas=(0.9, -0.1)), dict(betas=(0.9, nan)), dict(eps=0.0), dict(eps=-1e-8), dict(eps=nan), dict(eps=inf), dict(weight_decay=-1e-4),
           dict(weight_decay=inf), dict(weight_decay=nan), dict(decoupled=2), dict(decoupled=-1)]
    for kw in bad:
        with pytest.raises(ConvNetError, match="status -1"):
            net.set_adam(**kw)
        assert net.get_adam() == before, kw
    net.close()
    fresh = make_net(FUSED_HEAD)                         # a refused first call allocates nothing and selects nothing
    with pytest.raises(ConvNetError, match="status -1"):
        fresh.set_adam(betas=(1.0, 0.999))
    assert fresh.get_adam()["selected"] is False
    with pytest.raises(ConvNetError, match="status -6"):
        fresh.get_adam_state()
    fresh.close()


def test_thirty_adam_steps_halve_the_loss():
    """one fixed FUSED_HEAD batch, lr 1e-3, the He-normal start of test_gpu_convnet_sgd.py's oracle test: the last loss is below half the
    first.  (The f64 oracle with _adam_ref from the same start goes 3.69 -> 0.0023 monotonically: three orders of magnitude of room.)"""
    spec = FUSED_HEAD
    in_shape, layers, B = spec
    rng = np.random.default_rng(B)
    flat = oracle_params(rng, in_shape, layers)[2].astype(np.float32)
    net = make_net(spec)
    net.set_params(flat)
    net.set_adam()
    x = net.to_device(rng.standard_normal((B,) + in_shape).astype(np.float32))
    y = net.to_device(rng.integers(0, layers[-1][1], B).astype(np.int32))
    loss = zeros(net, 1)
    seen = []
    for _ in range(30):
        step(net, x, y, 1e-3, loss)
        seen.append(float(loss.cpu()[0]))
    print("loss", seen[0], "->", seen[-1])
    assert np.isfinite(seen).all() and seen[-1] < 0.5 * seen[0], (seen[0], seen[-1])
    assert net.get_adam_state()[2] == 30
    net.close()
