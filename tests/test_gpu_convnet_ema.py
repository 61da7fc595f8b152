"""GPU tests of Track X's average of the parameters (include/rcn_hipx.h, rcn_hipx_set_ema): the exponential moving average kept by the
step's one reduction launch (k_reduce_all_ema / _sgd_ema and their _dlr forms), its data-parallel half (k_ema_lerp), and the evaluation
on it (rcn_hipx_evaluate_ex_dev, k_swap4).

Every comparison is bit for bit.  The average's update has no fused multiply-add, so tests/_ema_ref.py (float32 NumPy, every operation
rounded once) reproduces it from the parameters a twin WITHOUT an average reads back after each step -- which also shows that switching
the average on changes no bit of the parameters or the velocity.  An evaluation on the average runs the launches of an evaluation on
the same bits held as live parameters, so it equals a twin's live evaluation after set_params(get_ema())."""
import ctypes as C

import numpy as np
import pytest
from _convnet_util import FUSED_HEAD, KW, LR, MOMENTUM, NESTEROV, PLAIN, PLAIN_HEAD, POOL_PAIRS, close, dev, epoch, make_net, random_set, step, sync, twins
from _ema_ref import ema_update

pytestmark = pytest.mark.gpu

DECAY = 0.5


def _batches(net, spec, n, seed=0, B=None):
    in_shape, layers, B0 = spec
    B = B or B0
    rng = np.random.default_rng(seed)
    return [(dev(net, rng.standard_normal((B,) + in_shape).astype(np.float32)), dev(net, rng.integers(0, layers[-1][1], B).astype(np.int32))) for _ in range(n)]


def _state(net):
    return net.get_params(), net.get_velocity(), net.get_ema()


def _same(s, t):
    return all(np.array_equal(u, v) for u, v in zip(s, t))


def _kernel(sgd, dlr=False):
    return "k_reduce_all" + ("_sgd" if sgd != PLAIN else "") + "_ema" + ("_dlr" if dlr else "") + ","


# ---- 1. the default is a net never configured ------------------------------------------------------------------------------------------

def test_decay_zero_is_a_net_never_configured():
    from mercer_research_amd.convnet import ConvNetError
    a, b = twins(FUSED_HEAD, "fp32", 2, PLAIN, configured_first=True)
    a.set_ema(0.0)
    assert a.get_ema_decay() == 0.0 and b.get_ema_decay() == 0.0
    B = FUSED_HEAD[2]
    assert a.plan_of_this_net(B) == b.plan_of_this_net(B) and "_ema" not in a.plan_of_this_net(B) and "EMA" not in a.plan_of_this_net(B)
    assert a.plan_epoch_of_this_net(B, "uint8", True) == b.plan_epoch_of_this_net(B, "uint8", True)
    p0 = a.get_params()
    x, y = _batches(a, FUSED_HEAD, 1)[0]
    for _ in range(4):                                   # eager, then graph replays
        step(a, x, y, LR)
        step(b, x, y, LR)
        assert np.array_equal(a.get_params(), b.get_params())
    assert not np.array_equal(a.get_params(), p0)
    assert a.graphs_instantiated() == b.graphs_instantiated()
    for n in (a, b):
        with pytest.raises(ConvNetError, match="status -6"):
            n.get_ema()
    a.close(); b.close()


# ---- 2. the fused step -----------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("spec,precision,sgd", [(FUSED_HEAD, "fp32", PLAIN), (PLAIN_HEAD, "fp32", NESTEROV), (FUSED_HEAD, "bf16", MOMENTUM),
                                                (POOL_PAIRS, "fp32", MOMENTUM), (POOL_PAIRS, "bf16_stored", MOMENTUM)],
                         ids=["fused_head-fp32-plain", "plain_head-fp32-nesterov", "fused_head-bf16-momentum", "pool_pairs-fp32-momentum", "pool_pairs-bf16_stored-momentum"])
def test_fused_step_keeps_the_average_and_changes_nothing_else(spec, precision, sgd):
    """Five steps: eager, graph replays, one step at a second lr (a second graph), and back to the first graph.  A has the average, twin B
    has not: the same parameters and velocity after every step, and A's average is the restatement applied to B's parameters."""
    a, b = twins(spec, precision, 2, sgd, configured_first=True)
    a.set_ema(DECAY)
    assert a.get_ema_decay() == DECAY
    plan = a.plan_of_this_net(spec[2])
    assert _kernel(sgd) in plan and "(EMA: decay 0.5)" in plan, plan
    assert "_ema" not in b.plan_of_this_net(spec[2])
    e = a.get_params()                                   # the start value: the live parameters when the average is switched on
    assert np.array_equal(a.get_ema(), e)
    x, y = _batches(a, spec, 1)[0]
    for k, lr in enumerate([0.05, 0.05, 0.05, 0.02, 0.05]):
        step(a, x, y, lr)
        step(b, x, y, lr)
        pb = b.get_params()
        e = ema_update(e, pb, DECAY)
        assert np.array_equal(a.get_params(), pb), k
        assert np.array_equal(a.get_velocity(), b.get_velocity()), k
        got = a.get_ema()
        assert np.array_equal(got, e), (k, float(np.abs(got - e).max()))
        if k >= 1:
            assert not np.array_equal(e, pb)             # the average is not the parameters: no equality above is vacuous
    if sgd[0]:
        assert np.abs(a.get_velocity()).max() > 0
    a.close(); b.close()


# ---- 3. the epoch path: the _dlr kernels and the mixed graphs ---------------------------------------------------------------------------

@pytest.mark.parametrize("sgd", [PLAIN, NESTEROV], ids=["plain", "nesterov"])
def test_epoch_with_schedule_augmentation_and_mixing_keeps_the_average(sgd):
    from mercer_research_amd.convnet import Augment, mix_plan
    spec = ((8, 8, 3), FUSED_HEAD[1], 8)
    B, nb, n = 8, 5, 40
    a, b = twins(spec, "fp32", 2, sgd, configured_first=True)
    a.set_ema(DECAY)
    plan = a.plan_epoch_of_this_net(B, "uint8", True, Augment(2, True, 3, 0), True)
    assert _kernel(sgd, dlr=True) in plan and "(EMA: decay 0.5)" in plan, plan
    X, y = random_set(a, spec, n, seed=7, u8=True)
    perm = dev(a, np.random.default_rng(8).permutation(n).astype(np.int32))
    rates = np.array([0.05, 0.05, 0.02, 0.05, 0.03], dtype=np.float32)
    lr = dev(a, rates)
    aug = Augment(2, True, 3, 0)
    rec = mix_plan(nb, 8, 8, mixup_alpha=0.8, cutmix_alpha=1.0, seed=5)
    rec[0] = (0.4, 0.4, 0, 0, 0, 0)                                  # whatever the draws are: one mixup step and one CutMix step
    rec[1] = (1.0, np.float32(1.0 - 6.0 / 64.0), 1, 3, 2, 5)
    recs = a.mix_to_device(rec)
    one = [b.mix_to_device(rec[s:s + 1]) for s in range(nb)]
    sync()
    e = a.get_params()
    ga, gb = a.graphs_instantiated(), b.graphs_instantiated()
    epoch(a, X, y, perm, B, lr, augment=aug, mix=recs, **KW)
    for s in range(nb):
        epoch(b, X, y, perm, B, lr[s:s + 1].contiguous(), first_batch=s, n_batches=1, augment=aug, mix=one[s], **KW)
        e = ema_update(e, b.get_params(), DECAY)
    assert np.array_equal(a.get_params(), b.get_params()) and np.array_equal(a.get_velocity(), b.get_velocity())
    got = a.get_ema()
    assert np.array_equal(got, e), float(np.abs(got - e).max())
    assert not np.array_equal(e, a.get_params())
    assert a.graphs_instantiated() - ga == b.graphs_instantiated() - gb
    # the un-mixed scheduled epoch (the other _dlr graph) goes on from there, bit for bit
    epoch(a, X, y, perm, B, lr, augment=aug, **KW)
    for s in range(nb):
        epoch(b, X, y, perm, B, lr[s:s + 1].contiguous(), first_batch=s, n_batches=1, augment=aug, **KW)
        e = ema_update(e, b.get_params(), DECAY)
    assert np.array_equal(a.get_params(), b.get_params()) and np.array_equal(a.get_velocity(), b.get_velocity())
    assert np.array_equal(a.get_ema(), e)
    assert a.graphs_instantiated() - ga == b.graphs_instantiated() - gb
    a.close(); b.close()


# ---- 4. the data-parallel half ---------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("sgd", [PLAIN, NESTEROV], ids=["plain-k_axpy", "nesterov-k_sgd_apply"])
def test_data_parallel_half_keeps_the_average_of_the_fused_step(sgd):
    """gradients on a twin + apply_sgd on A against train_step on a third net, two steps.  With the configured optimiser (k_sgd_apply, the
    fused update's own arithmetic) everything is bit for bit.  With the default one the update launch is k_axpy, whose arithmetic is not
    pinned to the fused launch's: the parameters are held to tests/test_gpu_convnet.py's rule for that comparison, and the average -- one
    rounding per operation in either launch -- to the restatement on that net's OWN parameters, bit for bit."""
    import torch
    spec = POOL_PAIRS
    a, twin, c = twins(spec, "fp32", 3, sgd, configured_first=True)
    a.set_ema(DECAY)
    c.set_ema(DECAY)
    x, y = _batches(a, spec, 1)[0]
    ea = ec = a.get_params()
    lr = 0.03
    for k in range(2):
        twin.set_params(a.get_params())
        with torch.cuda.stream(twin.stream):
            grad = twin.gradients(x, y)
        twin.synchronize()
        with torch.cuda.stream(a.stream):
            a.apply_sgd(grad, 1.0, lr)
        a.synchronize()
        step(c, x, y, lr)
        ea, ec = ema_update(ea, a.get_params(), DECAY), ema_update(ec, c.get_params(), DECAY)
        assert np.array_equal(a.get_ema(), ea) and np.array_equal(c.get_ema(), ec), k
        assert not np.array_equal(ea, a.get_params())
        if sgd == PLAIN:
            close(a.get_params(), c.get_params())
            close(a.get_ema(), c.get_ema())
        else:
            assert _same(_state(a), _state(c)), k
    # rcn_hipx_apply_dev stays the plain axpy: neither the velocity nor the average moves
    with torch.cuda.stream(a.stream):
        a.apply(grad, lr)
    a.synchronize()
    assert np.array_equal(a.get_ema(), ea) and np.array_equal(a.get_velocity(), c.get_velocity())
    assert not np.array_equal(a.get_params(), c.get_params())
    a.close(); twin.close(); c.close()


# ---- 5. evaluation on the average ------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("u8", [True, False], ids=["uint8", "float32"])
@pytest.mark.parametrize("spec,precision,max_batch,rows", [(FUSED_HEAD, "fp32", 16, 37), (FUSED_HEAD, "bf16", 16, 37), (POOL_PAIRS, "bf16_stored", 64, 150)],
                         ids=["fused_head-fp32", "fused_head-bf16", "pool_pairs-bf16_stored"])
def test_evaluation_on_the_average_is_a_twins_live_evaluation_and_leaves_training_alone(spec, precision, max_batch, rows, u8):
    """Two full chunks and a short one.  A and N train three steps with the average; A evaluates on it, N never evaluates."""
    a, n, twin = twins(spec, precision, 3, MOMENTUM, max_batch=max_batch, configured_first=True)
    for net in (a, n):
        net.set_ema(DECAY)
    batches = _batches(a, spec, 2, seed=3)
    for k in range(3):
        for net in (a, n):
            step(net, *batches[k % 2], LR)
    X, y = random_set(a, spec, rows, seed=9, u8=u8)
    before = _state(a)
    twin.set_params(before[2])
    g0 = a.graphs_instantiated()
    live = a.evaluate(X, y, **KW)
    got = a.evaluate(X, y, weights="ema", **KW)
    got_pred = a.predict(X, weights="ema", **KW)
    a.synchronize()
    ls, cs, ps = a.evaluate_async(X, y, weights="ema", **KW)
    a.synchronize()
    assert a.graphs_instantiated() == g0
    assert _same(_state(a), before)                      # the live parameters are back, bit for bit; velocity and average untouched
    want = twin.evaluate(X, y, **KW)
    want_pred = twin.predict(X, **KW)
    twin.synchronize()
    wl, wc, wp = twin.evaluate_async(X, y, **KW)
    twin.synchronize()
    assert got == want, (got, want)
    assert float(ls.item()) == float(wl.item()) and int(cs.item()) == int(wc.item())
    assert np.array_equal(got_pred.cpu().numpy(), want_pred.cpu().numpy()) and np.array_equal(ps.cpu().numpy(), wp.cpu().numpy())
    assert got[0] != live[0]                             # not the live parameters' loss
    assert a.evaluate(X, y, **KW) == live                # ... which the live path still returns
    # training goes on as if nothing had happened: a stale bf16 operand copy or a missed exchange would show here
    for k in range(3, 5):
        for net in (a, n):
            step(net, *batches[k % 2], LR)
        assert _same(_state(a), _state(n)), k
    assert not np.array_equal(a.get_ema(), a.get_params())
    a.close(); n.close(); twin.close()


# ---- 6. state --------------------------------------------------------------------------------------------------------------------------

def test_state_saved_and_loaded_continues_and_survives_and_changes_reach_the_replay():
    from mercer_research_amd.convnet import ConvNetError
    spec = FUSED_HEAD
    a, b = twins(spec, "fp32", 2, MOMENTUM, configured_first=True)
    for net in (a, b):
        net.set_ema(DECAY)
    batches = _batches(a, spec, 3, seed=4)
    for k in range(6):
        step(a, *batches[k % 3], LR)
    for k in range(3):
        step(b, *batches[k % 3], LR)
    p3, v3, e3 = _state(b)
    b.close()
    c = make_net(spec, "fp32", MOMENTUM)
    with pytest.raises(ConvNetError, match="status -6"):
        c.set_ema_params(e3)                             # no average yet
    c.reset_ema()                                        # ... and nothing to reset: a no-op
    c.set_params(p3)
    c.set_velocity(v3)
    c.set_ema(DECAY)
    assert np.array_equal(c.get_ema(), p3)               # the start value
    c.set_ema_params(e3)
    for k in range(3, 6):
        step(c, *batches[k % 3], LR)
    assert _same(_state(c), _state(a))
    # the average survives set_params, init_params and a change of precision
    e = c.get_ema()
    c.set_params(p3)
    c.init_params(7)
    c.set_precision("bf16")
    c.set_precision("fp32")
    assert np.array_equal(c.get_ema(), e) and not np.array_equal(e, c.get_params())
    c.reset_ema()
    c.synchronize()
    assert np.array_equal(c.get_ema(), c.get_params())
    # decay 0 on a net whose step is a captured graph: the updates stop (the replay does not touch the average), the buffer stays evaluable
    x, y = batches[0]
    for _ in range(3):
        step(c, x, y, LR)
    e = c.get_ema()
    assert not np.array_equal(e, c.get_params())
    c.set_ema(0.0)
    assert c.get_ema_decay() == 0.0 and "_ema" not in c.plan_of_this_net(spec[2])
    for _ in range(3):
        step(c, x, y, LR)
    assert np.array_equal(c.get_ema(), e)
    X, yy = random_set(c, spec, 11, seed=2)
    twin = make_net(spec, sgd=PLAIN)
    twin.set_params(e)
    assert c.evaluate(X, yy, weights="ema") == twin.evaluate(X, yy)
    # a changed decay reaches the step although (x, y, lr) has a captured graph: graphs that were not dropped would show here
    c.set_ema(0.75)
    for _ in range(3):
        step(c, x, y, LR)
        e = ema_update(e, c.get_params(), 0.75)
        assert np.array_equal(c.get_ema(), e)
    c.set_ema(0.25)
    step(c, x, y, LR)
    e = ema_update(e, c.get_params(), 0.25)
    assert np.array_equal(c.get_ema(), e) and c.get_ema_decay() == 0.25
    a.close(); c.close(); twin.close()


# ---- 7. refusals -----------------------------------------------------------------------------------------------------------------------

def test_refusals():
    import torch
    from mercer_research_amd.convnet import ConvNetError
    spec = POOL_PAIRS
    B = spec[2]
    net = make_net(spec, sgd=PLAIN)
    net.init_params(2)
    X, y = random_set(net, spec, B, seed=6)
    with pytest.raises(ConvNetError, match="status -6"):
        net.evaluate(X, y, weights="ema")                # no average
    with pytest.raises(ConvNetError, match="status -6"):
        net.predict(X, weights="ema")
    with pytest.raises(ValueError):
        net.evaluate(X, y, weights="swa")
    net.set_ema(0.25)
    for bad in (-0.1, 1.0, float("nan"), float("inf")):
        with pytest.raises(ConvNetError, match="status -1"):
            net.set_ema(bad)
        assert net.get_ema_decay() == 0.25
    with torch.cuda.stream(net.stream):
        loss_sum = torch.zeros(1, dtype=torch.float64, device=net.device)
        correct = torch.zeros(1, dtype=torch.int64, device=net.device)
        grad = torch.empty(net.n_padded, dtype=torch.float32, device=net.device)
    net.synchronize()
    p = net.get_params()
    for weights in (2, -1):
        assert net.lib.rcn_hipx_evaluate_ex_dev(net.net, C.c_void_p(X.data_ptr()), 0, 1.0, 0.0, C.c_void_p(y.data_ptr()), B, weights,
                                                C.c_void_p(loss_sum.data_ptr()), C.c_void_p(correct.data_ptr()), None) == -1
    # an open bucket walk: -6 in either mode, nothing exchanged
    nb, off, ln = C.c_int(), C.c_int64(), C.c_int64()
    net._ck(net.lib.rcn_hipx_gradients_begin_dev(net.net, C.c_void_p(X.data_ptr()), C.c_void_p(y.data_ptr()), B, C.c_void_p(grad.data_ptr()), None, 0, C.byref(nb)))
    assert nb.value >= 2
    net._ck(net.lib.rcn_hipx_gradients_bucket_dev(net.net, 0, C.byref(off), C.byref(ln)))
    for weights in ("live", "ema"):
        with pytest.raises(ConvNetError, match="status -6"):
            net.evaluate(X, y, weights=weights)
    for k in range(1, nb.value):
        net._ck(net.lib.rcn_hipx_gradients_bucket_dev(net.net, k, C.byref(off), C.byref(ln)))
    net.synchronize()
    assert np.array_equal(net.get_params(), p) and np.array_equal(net.get_ema(), p)
    net.evaluate(X, y, weights="ema")                    # the walk is over: evaluation runs again
    net.close()
