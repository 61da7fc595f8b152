"""GPU tests of Track-X gradient accumulation over micro-batches (include/rcn_hipx.h, rcn_hipx_set_accumulate): the two micro-step
reductions (k_reduce_all_acc<first|next>), the update over the accumulator as one-chunk slabs (with k_grad_sumsq in front of it where
clipping is on), the three kinds of captured graph, and the position in the cycle as host state of the net.

The twin-net method of tests/test_gpu_convnet_clip.py: net A takes the library's micro-steps; net B supplies gradients() of every
micro-batch at the same parameters (the same kernels and sums as the step); the host applies tests/_accum_ref.py, then _clip_ref, then
_sgd_ref.sgd_update / _clip_ref.plain_update and _ema_ref.ema_update.  Every micro-batch of a cycle holds different data: a step that
re-read one batch would otherwise pass."""
import numpy as np
import pytest
from _accum_ref import accumulate, scale_of
from _clip_ref import apply_coef, grad_norm, plain_update
from _convnet_util import (FUSED_HEAD, INF, NESTEROV, PLAIN, PLAIN_HEAD, POOL_PAIRS, batch, batches_by_seed, bits, check_norm, close, epoch, grad, make_net,
                           same_bits, same_state, step, twins)
from _ema_ref import ema_update
from _sgd_ref import sgd_update

from oracle import convnet_oracle as co

pytestmark = pytest.mark.gpu

LRS = [0.05, 0.05, 0.02]                                # three cycles: eager, replays, a second graph of the last kind
IGNORED = 1e3                                           # the rate handed to micro-steps that apply no update


def _host_update(p, v, e, acc, lr, sgd, decay, coef=None):
    g = acc if coef is None else apply_coef(acc, coef)
    if sgd == PLAIN:
        p = plain_update(p, g, lr)
    else:
        p, v = sgd_update(p, g, v, lr, *sgd)
    if decay:
        e = ema_update(e, p, decay)
    return p, v, e


def _cycle(a, b, batches, k, p, lr):
    """One cycle of k micro-steps on A with B's gradients at p beside it; checks every non-final micro-step; returns (acc logical, acc padded)"""
    v0, e0 = a.get_velocity(), (a.get_ema() if a.get_ema_decay() else None)
    logical, padded = [], []
    for j, (x, y) in enumerate(batches):
        gdev, gpad = grad(b, x, y, p)
        logical.append(b.unpad(gdev))
        padded.append(gpad)
        assert a.get_accumulate() == (k, j)
        step(a, x, y, lr if j == k - 1 else IGNORED)
        assert a.get_accumulate() == (k, (j + 1) % k)
        assert same_bits(a.get_accumulated(), accumulate(logical, k)), (j, float(np.abs(a.get_accumulated() - accumulate(logical, k)).max()))
        if j < k - 1:
            assert same_bits(a.get_params(), p), j
            assert same_bits(a.get_velocity(), v0), j
            if e0 is not None:
                assert same_bits(a.get_ema(), e0), j
    return accumulate(logical, k), accumulate(padded, k)


def _check_against_host(spec, precision, k, sgd, decay=0.0, clip=False):
    a, b = twins(spec, precision)
    a.set_sgd(*sgd)
    if decay:
        a.set_ema(decay)
    a.set_accumulate(k)
    assert a.get_accumulate() == (k, 0)
    batches = batches_by_seed(a, spec, k)
    p = a.get_params()
    v, e = np.zeros(a.n_logical, dtype=np.float32), p.copy()
    max_norm = None
    if clip:
        first = accumulate([grad(b, x, y, p)[1] for x, y in batches], k)
        max_norm = float(grad_norm(first) / np.float32(2))          # half the first cycle's norm of acc
        a.set_clip(max_norm)
        assert a.get_accumulate() == (k, 0)
    g0 = a.graphs_instantiated()
    for cyc, lr in enumerate(LRS):
        count = a.grad_norm_count() if clip else 0
        acc, acc_pad = _cycle(a, b, batches, k, p, lr)
        coef = None
        if clip:
            norm, coef = a.grad_norm()
            check_norm(f"cycle {cyc}", norm, coef, grad_norm(acc_pad), max_norm)
            assert cyc > 0 or coef < 1.0
            assert a.grad_norm_count() == count + 1 == cyc + 1      # updates, not micro-steps
        p, v, e = _host_update(p, v, e, acc, lr, sgd, decay, coef)
        assert same_bits(a.get_params(), p), (cyc, float(np.abs(a.get_params() - p).max()))
        assert same_bits(a.get_velocity(), v), cyc
        if decay:
            assert same_bits(a.get_ema(), e), cyc
    # one graph per kind of micro-step (and tensors), the last kind once per host rate
    assert a.graphs_instantiated() == g0 + k + 1
    a.close(); b.close()


def test_off_is_off():
    from mercer_research_amd.convnet import ConvNetError
    a, b = twins(FUSED_HEAD, "fp32")
    a.set_accumulate(1)
    assert a.get_accumulate() == (1, 0)
    B = FUSED_HEAD[2]
    assert a.plan_of_this_net(B) == b.plan_of_this_net(B)
    assert a.plan_epoch_of_this_net(B, lr_from_device=True) == b.plan_epoch_of_this_net(B, lr_from_device=True)
    assert "accumulate" not in a.plan_of_this_net(B) and "k_reduce_all_acc" not in a.plan_of_this_net(B)
    with pytest.raises(ConvNetError, match="-1"):
        a.plan_micro_of_this_net(B, "first")
    x, y = batch(a, FUSED_HEAD)
    p0 = a.get_params()
    for _ in range(4):                                   # eager, then graph replays
        step(a, x, y, 0.05)
        step(b, x, y, 0.05)
        assert a.get_accumulate() == (1, 0)
    assert same_bits(a.get_params(), b.get_params()) and not same_bits(a.get_params(), p0)
    assert a.graphs_instantiated() == b.graphs_instantiated() == 1
    with pytest.raises(ConvNetError, match="status -6"):
        a.get_accumulated()
    a.reset_accumulation()
    a.close(); b.close()


@pytest.mark.parametrize("k", [2, 3])
@pytest.mark.parametrize("sgd", [PLAIN, NESTEROV], ids=["default", "nesterov"])
@pytest.mark.parametrize("spec,precision", [(FUSED_HEAD, "fp32"), (PLAIN_HEAD, "fp32"), (FUSED_HEAD, "bf16"), (POOL_PAIRS, "bf16_stored")],
                         ids=["fused_head-fp32", "plain_head-fp32", "fused_head-bf16", "pool_pairs-bf16_stored"])
def test_accumulated_update_is_the_host_update_bit_for_bit(spec, precision, sgd, k):
    _check_against_host(spec, precision, k, sgd)


@pytest.mark.parametrize("k", [2, 3])
def test_with_the_average(k):
    _check_against_host(FUSED_HEAD, "fp32", k, NESTEROV, decay=0.9)


@pytest.mark.parametrize("k", [2, 3])
@pytest.mark.parametrize("sgd,decay", [(PLAIN, 0.0), (NESTEROV, 0.9)], ids=["default", "nesterov-ema"])
def test_with_clipping(sgd, decay, k):
    _check_against_host(FUSED_HEAD, "fp32", k, sgd, decay=decay, clip=True)


@pytest.mark.parametrize("sgd", [PLAIN, NESTEROV], ids=["default", "nesterov"])
def test_measure_only_leaves_the_unclipped_accumulating_twin(sgd):
    spec, k = PLAIN_HEAD, 2
    a, u = twins(spec, "fp32")
    for n in (a, u):
        n.set_sgd(*sgd)
        n.set_accumulate(k)
    a.set_clip(INF)
    batches = batches_by_seed(a, spec, k)
    for cyc in range(2):
        for x, y in batches:
            step(a, x, y, 0.05)
            step(u, x, y, 0.05)
        assert a.grad_norm()[1] == 1.0 and a.grad_norm_count() == cyc + 1
        assert same_bits(a.get_params(), u.get_params()) and same_bits(a.get_velocity(), u.get_velocity()), cyc
    assert same_bits(a.get_accumulated(), u.get_accumulated())
    a.close(); u.close()


def test_one_cycle_against_the_f64_oracle_on_the_concatenated_batch():
    """k = 3 micro-batches of 5 rows, plain SGD: the parameters after the cycle are the oracle's step on the 15 rows (a cycle adds k
    roundings of 2^-24 each to the one step tests/test_gpu_convnet.py allows 2e-4)"""
    in_shape, layers, B = FUSED_HEAD
    k, lr = 3, 0.05
    rng = np.random.default_rng(15)
    net = make_net(FUSED_HEAD)
    shapes = co.param_shapes(in_shape, layers)
    ws = [rng.standard_normal(s) * np.sqrt(2.0 / s[0]) for s, _ in shapes]
    bs = [rng.standard_normal(n) * 0.1 for _, n in shapes]
    net.set_params(co.flatten(ws, bs))
    x = rng.standard_normal((k * B,) + in_shape).astype(np.float32)
    y = rng.integers(0, layers[-1][1], k * B).astype(np.int32)
    w32 = [w.astype(np.float32).astype(np.float64) for w in ws]
    b32 = [b.astype(np.float32).astype(np.float64) for b in bs]
    nw, nb, _ = co.sgd_step(x.astype(np.float64), y, w32, b32, layers, lr)
    net.set_accumulate(k)
    parts = [(net.to_device(x[j * B:(j + 1) * B]), net.to_device(y[j * B:(j + 1) * B])) for j in range(k)]
    net.synchronize()
    for xd, yd in parts:
        step(net, xd, yd, lr)
    assert net.get_accumulate() == (k, 0)
    err = float(np.abs(net.get_params().astype(np.float64) - co.flatten(nw, nb)).max())
    print(f"max |device - oracle| after one cycle of {k}: {err:.3e}")
    close(net.get_params(), co.flatten(nw, nb))
    net.close()


@pytest.mark.parametrize("clip", [False, True], ids=["nesterov", "nesterov-clipped"])
def test_data_parallel_identity(clip):
    """apply_sgd(acc uploaded in the padded layout, 1, lr) on a twin that does not accumulate holds the accumulating net's parameters and
    velocity bit for bit"""
    import torch
    spec, k, lr = FUSED_HEAD, 2, 0.03
    a, b, d = twins(spec, "fp32", 3)
    batches = batches_by_seed(a, spec, k)
    p0 = a.get_params()
    for n in (a, d):
        n.set_sgd(*NESTEROV)
    if clip:
        first = accumulate([grad(b, x, y, p0)[1] for x, y in batches], k)
        max_norm = float(grad_norm(first) / np.float32(2))
        for n in (a, d):
            n.set_clip(max_norm)
    a.set_accumulate(k)
    for cyc in range(2):                                 # the second cycle on a velocity that is not zero
        p = a.get_params()
        acc_pad = accumulate([grad(b, x, y, p)[1] for x, y in batches], k)
        for x, y in batches:
            step(a, x, y, lr)
        acc_dev = d.to_device(acc_pad)
        d.synchronize()
        assert acc_dev.data_ptr() % 16 == 0 and same_bits(d.unpad(acc_dev), a.get_accumulated())
        with torch.cuda.stream(d.stream):
            d.apply_sgd(acc_dev, 1.0, lr)
        d.synchronize()
        if clip:
            assert a.grad_norm() == d.grad_norm() and (cyc > 0 or a.grad_norm()[1] < 1.0)
        assert same_bits(a.get_params(), d.get_params()) and not same_bits(a.get_params(), p), cyc
        assert same_bits(a.get_velocity(), d.get_velocity()), cyc
    a.close(); b.close(); d.close()


# ---- the epoch entries ---------------------------------------------------------------------------------------------------------------------
ROWS, EB, NB = 24, 4, 6                                 # a uint8 set of 24 rows, micro-batches of 4: six of them
RATES = np.array([0.01, 0.03, 0.05, 0.04, 0.02, 0.06], dtype=np.float32)


def _set(net, seed=6):
    in_shape, layers, _ = FUSED_HEAD
    rng = np.random.default_rng(seed)
    X = net.to_device(rng.integers(0, 256, (ROWS,) + in_shape).astype(np.uint8))
    Y = net.to_device(rng.integers(0, layers[-1][1], ROWS).astype(np.int32))
    perm = net.to_device(rng.permutation(ROWS).astype(np.int32))
    net.synchronize()
    return X, Y, perm


def _epoch_twins(count, k):
    nets = twins(FUSED_HEAD, "fp32", count)
    for n in nets:
        n.set_sgd(*NESTEROV)
        n.set_accumulate(k)
    return nets


@pytest.mark.parametrize("k", [2, 3])
def test_epoch_is_the_micro_batches_fed_one_by_one(k):
    """... bit for bit, losses per micro-batch included; k graphs for the first epoch, none for a second one with another schedule; the
    rates of the micro-steps that apply no update are ignored"""
    import torch
    a, t, c = _epoch_twins(3, k)
    X, Y, perm = _set(a)
    p0 = a.get_params()
    lr = a.to_device(RATES)
    la = torch.zeros(NB, dtype=torch.float32, device=a.device)
    a.synchronize()
    g0 = a.graphs_instantiated()
    epoch(a, X, Y, perm, EB, lr, losses=la)
    assert a.graphs_instantiated() == g0 + k
    assert a.get_accumulate() == (k, NB % k) == (k, 0)
    lt = torch.zeros(NB, dtype=torch.float32, device=t.device)
    keep = []
    with torch.cuda.stream(t.stream):
        for s in range(NB):
            x, y = t.gather_batch(X, Y, perm[s * EB:(s + 1) * EB].contiguous(), EB)
            keep.append((x, y))
            t.train_step(x, y, float(RATES[s]), lt[s:s + 1])
    t.synchronize()
    assert same_state(a, t) and not same_bits(a.get_params(), p0)
    assert same_bits(a.get_accumulated(), t.get_accumulated())
    losses = la.cpu().numpy()
    assert np.array_equal(bits(losses), bits(lt.cpu().numpy())), (losses, lt.cpu().numpy())
    assert np.all(np.isfinite(losses)) and np.all(losses > 0) and len(set(losses.tolist())) == NB      # every micro-batch's own loss
    # the rates of the micro-steps that apply no update: not one bit changes
    junk = RATES.copy()
    junk[[s for s in range(NB) if s % k != k - 1]] = IGNORED
    epoch(c, X, Y, perm, EB, c.to_device(junk))
    assert same_state(a, c)
    # a second epoch with another schedule: no new graph
    lr2 = a.to_device((RATES[::-1] * np.float32(0.5)).astype(np.float32))
    epoch(a, X, Y, perm, EB, lr2)
    assert a.graphs_instantiated() == g0 + k
    for n in (a, t, c):
        n.close()


def test_epoch_split_calls_and_a_pending_tail():
    k = 2
    a, s, r, w = _epoch_twins(4, k)
    X, Y, perm = _set(a)
    lr = a.to_device(RATES)
    a.synchronize()
    epoch(a, X, Y, perm, EB, lr)
    # 3 + 3 micro-batches: the first call ends inside a cycle
    epoch(s, X, Y, perm, EB, lr[:3].contiguous(), n_batches=3)
    assert s.get_accumulate() == (k, 1)
    epoch(s, X, Y, perm, EB, lr[3:].contiguous(), first_batch=3, n_batches=3)
    assert s.get_accumulate() == (k, 0) and same_state(a, s)
    # five micro-batches leave one pending; reset_accumulation drops it: the next cycle is that of a twin that never saw the fifth
    epoch(r, X, Y, perm, EB, lr, n_batches=5)
    epoch(w, X, Y, perm, EB, lr, n_batches=4)
    assert r.get_accumulate() == (k, 1) and w.get_accumulate() == (k, 0) and same_state(r, w)
    r.reset_accumulation()
    assert r.get_accumulate() == (k, 0)
    for n in (r, w):
        epoch(n, X, Y, perm, EB, lr, n_batches=2)
    assert same_state(r, w) and same_bits(r.get_accumulated(), w.get_accumulated())
    for n in (a, s, r, w):
        n.close()


def test_mixed_epoch_is_gather_mix_and_train_step_pair_one_by_one():
    import torch
    from mercer_research_amd.convnet import mix_plan
    k = 2
    (H, W, _), _, _ = FUSED_HEAD
    a, t = _epoch_twins(2, k)
    X, Y, perm = _set(a)
    rec = mix_plan(NB, H, W, mixup_alpha=0.8, cutmix_alpha=1.0, seed=5)
    rec[0] = (0.4, 0.4, 0, 0, 0, 0)                                  # whatever the draws are: one mixup step and one CutMix step
    rec[1] = (1.0, np.float32(1.0 - 6.0 / (H * W)), 1, 3, 2, 5)
    recs = a.mix_to_device(rec)
    lr = a.to_device(RATES)
    la = torch.zeros(NB, dtype=torch.float32, device=a.device)
    a.synchronize()
    g0 = a.graphs_instantiated()
    epoch(a, X, Y, perm, EB, lr, losses=la, mix=recs)
    assert a.graphs_instantiated() == g0 + k
    lt = torch.zeros(NB, dtype=torch.float32, device=t.device)
    keep = []
    with torch.cuda.stream(t.stream):
        for s in range(NB):
            x, ya, yb = t.gather_mix(X, Y, perm[s * EB:(s + 1) * EB].contiguous(), EB, recs[s:s + 1], q0=s * EB)
            wgt = torch.tensor([float(rec["weight"][s])], dtype=torch.float32, device=t.device)
            keep.append((x, ya, yb, wgt))
            t.train_step_pair(x, ya, yb, wgt, float(RATES[s]), lt[s:s + 1])
    t.synchronize()
    assert same_state(a, t)
    assert np.array_equal(bits(la.cpu().numpy()), bits(lt.cpu().numpy()))
    a.close(); t.close()


# ---- state -----------------------------------------------------------------------------------------------------------------------------------
def test_state():
    from mercer_research_amd.convnet import ConvNetError
    spec = FUSED_HEAD
    B = spec[2]
    a, f, c = twins(spec, "fp32", 3)
    for n in (a, f, c):
        n.set_sgd(*NESTEROV)
    xs = batches_by_seed(a, spec, 3)
    X, Y, _ = _set(a)
    # refusals change nothing
    a.set_accumulate(3)
    graphs = a.graphs_instantiated()
    for bad in (0, -1, 65537):
        with pytest.raises(ConvNetError, match="status -1"):
            a.set_accumulate(bad)
        assert a.get_accumulate() == (3, 0)
    # the plans
    first, middle, last = (a.plan_micro_of_this_net(B, kind) for kind in ("first", "middle", "last"))
    assert "k_reduce_all_acc<first>" in first and "k_reduce_all_acc<next>" not in first and "update:" not in first
    assert "k_reduce_all_acc<next>" in middle and "k_reduce_all_acc<first>" not in middle and "update:" not in middle
    assert "(accumulate: micro-batch of 3, no update)" in first and "(accumulate: micro-batch of 3, no update)" in middle
    assert "k_reduce_all_acc<next>" in last and "update: k_reduce_all_sgd," in last and "as one-chunk slabs" in last
    plan = a.plan_of_this_net(B)
    assert plan == last
    update = [line for line in plan.splitlines() if line.lstrip().startswith("update:")]
    assert len(update) == 1 and "(accumulate: 3 micro-batches, scale %g)" % float(scale_of(3)) in update[0], plan
    epoch_plan = a.plan_epoch_of_this_net(B, lr_from_device=True)
    assert "k_reduce_all_acc<next>" in epoch_plan and "update: k_reduce_all_sgd_dlr," in epoch_plan and "accumulate: 3 micro-batches" in epoch_plan
    assert "graph: one graph per kind of micro-step (first, middle, last) and B; the last kind with lr from device" in epoch_plan, epoch_plan
    assert "graph: one graph per B" not in epoch_plan and "the last kind per (B, lr)" in a.plan_epoch_of_this_net(B)
    with pytest.raises(ValueError):
        a.plan_micro_of_this_net(B, "whole")
    # a changed k with a cycle open discards it: the next update is a fresh twin's
    step(a, *xs[0], 0.05)
    assert a.get_accumulate() == (3, 1) and a.graphs_instantiated() == graphs + 1
    a.set_accumulate(3)                                  # the k it has: a no-op
    assert a.get_accumulate() == (3, 1) and a.graphs_instantiated() == graphs + 1
    a.set_accumulate(2)
    assert a.get_accumulate() == (2, 0)
    assert "(first, last) and B" in a.plan_epoch_of_this_net(B)
    for n in (f, c):
        n.set_accumulate(2)
    for x, y in xs[1:]:
        for n in (a, f, c):
            step(n, x, y, 0.05)
    assert a.get_accumulate() == (2, 0) and same_state(a, f)
    # evaluation, set_params and a change of precision between two micro-steps: acc and the position stay, and so does the cycle's result
    p = a.get_params()
    step(a, *xs[0], IGNORED)
    step(c, *xs[0], IGNORED)                            # (c: the same cycle without the calls in between)
    acc = a.get_accumulated()
    assert a.evaluate(X, Y) == f.evaluate(X, Y)
    assert same_bits(a.get_accumulated(), acc) and a.get_accumulate() == (2, 1)
    a.set_params(p)
    a.set_precision("bf16")
    a.set_precision("fp32")
    assert same_bits(a.get_accumulated(), acc) and a.get_accumulate() == (2, 1) and same_bits(a.get_params(), p)
    step(a, *xs[2], 0.02)
    step(c, *xs[2], 0.02)
    assert a.get_accumulate() == (2, 0) and same_state(a, c) and not same_bits(a.get_params(), p)
    # back to 1: the whole step again, the accumulator kept
    a.set_accumulate(1)
    c.set_accumulate(1)
    acc = a.get_accumulated()
    step(a, *xs[0], 0.05)
    step(c, *xs[0], 0.05)
    assert same_state(a, c) and same_bits(a.get_accumulated(), acc) and a.get_accumulate() == (1, 0)
    for n in (a, f, c):
        n.close()
