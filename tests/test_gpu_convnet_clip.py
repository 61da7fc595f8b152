"""GPU tests of Track-X gradient clipping by global norm (include/rcn_hipx.h, rcn_hipx_set_clip): the three launches of the clipped
reduction (k_reduce_all into the net's gradient buffer, k_grad_sumsq, k_reduce_all_clip...), the data-parallel half (k_sgd_apply_clip),
the norm on its own (rcn_hipx_grad_norm_dev) and the ring log.

The twin-net method of tests/test_gpu_convnet_sgd.py: net A takes the library's step; net B supplies gradients() at the same parameters
(the same kernels and sums as the step); the host applies tests/_clip_ref.py, then _sgd_ref.sgd_update and _ema_ref.ema_update.  For the
coefficient the host uses the value the device reports, and three things are asserted: the device's coef is clip_coef(norm_dev, max_norm)
bit for bit; norm_dev is within one float32 ulp of the restatement's norm of B's gradient (whether it was exact is printed: the double
square root's last bit on the device is the one thing the restatement cannot promise); parameters, velocity and average are equal bit for bit."""
import numpy as np
import pytest
from _clip_ref import apply_coef, grad_norm, plain_update
from _convnet_util import FUSED_HEAD, INF, MU, PLAIN, PLAIN_HEAD, POOL_PAIRS, WD, batch, check_norm, grad, make_net, same_bits, step, twins
from _ema_ref import ema_update
from _sgd_ref import sgd_update

pytestmark = pytest.mark.gpu

LRS = [0.05, 0.05, 0.05, 0.02, 0.05]                   # eager, replays, a second graph, back to the first


def _host_step(b, x, y, p, v, e, lr, coef, sgd, decay, scale=1.0):
    """B's gradient at p, clipped by the device's coefficient, then the float32 restatements of the update and the average"""
    gdev, gpad = grad(b, x, y, p)
    g = apply_coef(b.unpad(gdev), coef, scale)
    if sgd == PLAIN:
        p = plain_update(p, g, lr)                       # (the default optimiser rounds p - lr g once: _clip_ref.plain_update)
    else:
        p, v = sgd_update(p, g, v, lr, *sgd)
    if decay:
        e = ema_update(e, p, decay)
    return p, v, e, grad_norm(gpad, scale)


def test_off_is_off():
    a, b = twins(FUSED_HEAD, "fp32")
    from mercer_research_amd.convnet import ConvNetError
    a.set_clip(0.0)
    assert a.get_clip() == 0.0
    B = FUSED_HEAD[2]
    assert a.plan_of_this_net(B) == b.plan_of_this_net(B)
    assert a.plan_epoch_of_this_net(B, lr_from_device=True) == b.plan_epoch_of_this_net(B, lr_from_device=True)
    assert "clip" not in a.plan_of_this_net(B) and "k_grad_sumsq" not in a.plan_of_this_net(B)
    x, y = batch(a, FUSED_HEAD)
    p0 = a.get_params()
    for _ in range(4):                                   # eager, then graph replays
        step(a, x, y, 0.05)
        step(b, x, y, 0.05)
    assert same_bits(a.get_params(), b.get_params()) and not same_bits(a.get_params(), p0)
    assert a.graphs_instantiated() == b.graphs_instantiated()
    with pytest.raises(ConvNetError, match="status -6"):
        a.grad_norm()
    assert a.grad_norm_count() == 0
    a.close(); b.close()


@pytest.mark.parametrize("sgd", [PLAIN, (MU, WD, True)], ids=["default", "nesterov"])
def test_measure_only_changes_no_bit(sgd):
    """max_norm = +inf: coef == 1 and the parameters of an unclipped twin, with the default optimiser too -- the clipped launches are
    instantiated on the unclipped launches' own functors (PlainUpdate rounds p - lr g once, SgdUpdate with mu = wd = 0 twice: they cannot
    share one)."""
    spec = FUSED_HEAD
    a, u, b = twins(spec, "fp32", 3)
    for n in (a, u):
        n.set_sgd(*sgd)
    a.set_clip(INF)
    assert a.get_clip() == INF
    x, y = batch(a, spec)
    for k, lr in enumerate(LRS):
        p = a.get_params()
        _, gpad = grad(b, x, y, p)
        step(a, x, y, lr)
        step(u, x, y, lr)
        norm, coef = a.grad_norm()
        assert coef == 1.0
        check_norm(f"measure-only step {k}", norm, coef, grad_norm(gpad), INF)
        assert same_bits(a.get_params(), u.get_params()), k
        assert same_bits(a.get_velocity(), u.get_velocity()), k
    assert a.grad_norm_count() == len(LRS)
    assert a.graphs_instantiated() == u.graphs_instantiated()
    a.close(); u.close(); b.close()


def _check_clipped_against_host(spec, precision, nesterov, decay, sgd=None):
    a, b = twins(spec, precision)
    sgd = sgd or (MU, WD, nesterov)
    a.set_sgd(*sgd)
    if decay:
        a.set_ema(decay)
    x, y = batch(a, spec)
    p = a.get_params()
    v, e = np.zeros(a.n_logical, dtype=np.float32), p.copy()
    max_norm = float(grad_norm(grad(b, x, y, p)[1]) / np.float32(2))       # half the first step's norm
    a.set_clip(max_norm)
    assert a.get_clip() == np.float32(max_norm)
    plan = a.plan_of_this_net(spec[2])
    assert "k_grad_sumsq" in plan and "k_reduce_all_clip" in plan and "clip: max norm" in plan, plan
    kernel = "k_reduce_all_clip" + ("_sgd" if sgd != PLAIN else "") + ("_ema" if decay else "") + ","
    assert kernel in plan, (kernel, plan)
    assert "(clip: max norm %g)" % max_norm in plan, plan
    for k, lr in enumerate(LRS):
        step(a, x, y, lr)
        norm, coef = a.grad_norm()
        p, v, e, norm_ref = _host_step(b, x, y, p, v, e, lr, coef, sgd, decay)
        check_norm(f"step {k}", norm, coef, norm_ref, max_norm)
        if k == 0:
            assert coef < 1.0
        assert same_bits(a.get_params(), p), (k, float(np.abs(a.get_params() - p).max()))
        assert same_bits(a.get_velocity(), v), k
        if decay:
            assert same_bits(a.get_ema(), e), k
    a.close(); b.close()


@pytest.mark.parametrize("nesterov", [False, True])
@pytest.mark.parametrize("spec,precision", [(FUSED_HEAD, "fp32"), (PLAIN_HEAD, "fp32"), (FUSED_HEAD, "bf16"), (PLAIN_HEAD, "bf16"), (POOL_PAIRS, "bf16_stored")],
                         ids=["fused_head-fp32", "plain_head-fp32", "fused_head-bf16", "plain_head-bf16", "pool_pairs-bf16_stored"])
def test_clipped_step_is_the_host_update_bit_for_bit(spec, precision, nesterov):
    _check_clipped_against_host(spec, precision, nesterov, 0.0)


def test_clipped_step_with_the_average():
    _check_clipped_against_host(FUSED_HEAD, "fp32", True, 0.9)


@pytest.mark.parametrize("decay", [0.0, 0.9], ids=["plain", "ema"])
def test_clipped_step_of_the_default_optimiser(decay):
    """plain SGD behind the coefficient: p - lr g' rounded once, as k_reduce_all rounds it (_clip_ref.plain_update)"""
    _check_clipped_against_host(PLAIN_HEAD, "fp32", False, decay, sgd=PLAIN)


@pytest.mark.parametrize("decay", [0.0, 0.9], ids=["plain", "ema"])
def test_one_graph_epoch_with_device_rate_and_ring_log(decay):
    """Six steps of train_epoch with the rate from a device tensor and a log of four slots against the same batches fed one by one to a twin
    (gather_batch + train_step + grad_norm): the norms of steps 2 .. 5 at k % 4, the parameters, one graph for both epochs."""
    import torch
    spec = FUSED_HEAD
    in_shape, layers, B = spec
    a, t, b = twins(spec, "fp32", 3)
    rng = np.random.default_rng(6)
    X = a.to_device(rng.integers(0, 256, (6 * B,) + in_shape).astype(np.uint8))
    Y = a.to_device(rng.integers(0, 10, 6 * B).astype(np.int32))
    rates = np.array([0.01, 0.03, 0.05, 0.04, 0.02, 0.01], dtype=np.float32)
    lr = a.to_device(rates)
    log = a.to_device(np.full(4, -1.0, dtype=np.float32))
    a.synchronize()
    with torch.cuda.stream(b.stream):
        x0, y0 = b.gather_batch(X, Y, None, B)
    max_norm = float(grad_norm(grad(b, x0, y0)[1]) / np.float32(2))
    for n in (a, t):
        n.set_sgd(MU, WD, True)
        if decay:
            n.set_ema(decay)
        n.set_clip(max_norm)
    a.set_grad_norm_log(log)
    plan = a.plan_epoch_of_this_net(B, lr_from_device=True)
    assert ("k_reduce_all_clip_sgd_ema_dlr," if decay else "k_reduce_all_clip_sgd_dlr,") in plan and "k_grad_sumsq" in plan and "clip: max norm" in plan, plan
    g0 = a.graphs_instantiated()
    with torch.cuda.stream(a.stream):
        a.train_epoch(X, Y, None, B, lr)
    a.synchronize()
    assert a.grad_norm_count() == 6
    assert a.graphs_instantiated() == g0 + 1
    norms = []
    for s in range(6):
        with torch.cuda.stream(t.stream):
            x, y = t.gather_batch(X, Y, None, B, base=s * B)
            t.train_step(x, y, float(rates[s]))
        norms.append(np.float32(t.grad_norm()[0]))
    assert norms[0] > np.float32(max_norm)               # clipping bites on the first step at least
    got = log.cpu().numpy()
    want = np.array([norms[4], norms[5], norms[2], norms[3]], dtype=np.float32)      # step k in slot k % 4
    assert np.array_equal(got.view(np.uint32), want.view(np.uint32)), (got, want)
    assert a.grad_norm()[0] == norms[5]
    assert same_bits(a.get_params(), t.get_params()) and same_bits(a.get_velocity(), t.get_velocity())
    if decay:
        assert same_bits(a.get_ema(), t.get_ema())
    with torch.cuda.stream(a.stream):
        a.train_epoch(X, Y, None, B, lr)
    a.synchronize()
    assert a.graphs_instantiated() == g0 + 1 and a.grad_norm_count() == 12
    a.set_grad_norm_log(None)
    assert a.grad_norm_count() == 0
    a.close(); t.close(); b.close()


@pytest.mark.parametrize("precision", ["fp32", "bf16_stored"])
def test_data_parallel_half(precision):
    """gradients + apply_sgd(grad, 1, lr) is the fused clipped step bit for bit; with grad_scale = 0.5 it is the host restatement at
    scale = 0.5; with the default optimiser and clipping on, apply_sgd still clips (it does not take the axpy)."""
    import torch
    spec = POOL_PAIRS
    a, b, c, d = twins(spec, precision, 4)
    sgd = (MU, WD, True)
    x, y = batch(a, spec)
    p0 = a.get_params()
    max_norm = float(grad_norm(grad(b, x, y)[1]) / np.float32(2))
    for n in (a, b, c):
        n.set_sgd(*sgd)
        n.set_ema(0.9)
    for n in (a, b, c, d):
        n.set_clip(max_norm)
    lr = 0.03
    for k in range(3):
        step(a, x, y, lr)
        with torch.cuda.stream(b.stream):
            g = b.gradients(x, y)
            b.apply_sgd(g, 1.0, lr)
        b.synchronize()
        assert a.grad_norm() == b.grad_norm() and (k > 0 or a.grad_norm()[1] < 1.0)
        assert same_bits(a.get_params(), b.get_params()) and same_bits(a.get_velocity(), b.get_velocity()) and same_bits(a.get_ema(), b.get_ema()), k
    assert b.grad_norm_count() == 3
    # grad_scale = 0.5 on c (first step: v = 0, e = p0); d: the default optimiser
    for net, opt, decay in ((c, sgd, 0.9), (d, PLAIN, 0.0)):
        with torch.cuda.stream(net.stream):
            g = net.gradients(x, y)
            net.apply_sgd(g, 0.5, lr)
        net.synchronize()
        norm, coef = net.grad_norm()
        gpad = g.cpu().numpy()
        check_norm(f"apply_sgd scale 0.5 {opt}", norm, coef, grad_norm(gpad, 0.5), max_norm)
        gc = apply_coef(net.unpad(g), coef, 0.5)
        p, v = sgd_update(p0, gc, np.zeros_like(p0), lr, *opt) if decay else (plain_update(p0, gc, lr), None)
        assert same_bits(net.get_params(), p)
        if decay:
            assert same_bits(net.get_velocity(), v) and same_bits(net.get_ema(), ema_update(p0, p, decay))
        else:
            assert coef < 1.0 and not same_bits(p, sgd_update(p0, net.unpad(g), np.zeros_like(p0), lr, grad_scale=0.5)[0])      # (the axpy's result)
    for n in (a, b, c, d):
        n.close()


@pytest.fixture(scope="module")
def norm_net():
    net = make_net(PLAIN_HEAD)
    yield net
    net.close()


@pytest.fixture(scope="module")
def norm_inputs():
    """one random buffer of the largest size; every case takes a prefix, and its restatement is computed once"""
    rng = np.random.default_rng(9)
    return (rng.standard_normal(4096 * 1030) * 0.3).astype(np.float32), {}


@pytest.mark.parametrize("scale", [1.0, 0.25])
@pytest.mark.parametrize("n", [0, 4, 4096, 4100, 4096 * 1030])
def test_the_norm_on_its_own(norm_net, norm_inputs, n, scale):
    import torch
    full, cache = norm_inputs
    net = norm_net
    g = full[:n]
    dev = net.to_device(g) if n else torch.empty(0, dtype=torch.float32, device=net.device)
    net.synchronize()
    out = net.grad_norm_of(dev, scale)
    net.synchronize()
    got = np.float32(out.item())
    if (n, scale) not in cache:
        cache[(n, scale)] = grad_norm(g, scale)
    ref = cache[(n, scale)]
    print(f"n {n} scale {scale}: device {got!r} restatement {ref!r} {'exact' if got == ref else 'differs'}")
    if n == 0:
        assert got == 0.0 and ref == 0.0
        return
    assert abs(float(got) - float(ref)) <= float(np.spacing(ref))
    exact = float(np.sqrt(np.sum((np.float32(scale) * g).astype(np.float64) ** 2)))
    assert abs(float(got) - exact) <= 2.0 ** -23 * exact
    assert net.get_clip() == 0.0                         # works with clipping off, and leaves it off


def test_the_norm_refuses_odd_sizes_and_misaligned_buffers(norm_net):
    from mercer_research_amd.convnet import ConvNetError
    net = norm_net
    buf = net.to_device(np.ones(16, dtype=np.float32))
    net.synchronize()
    assert buf.data_ptr() % 16 == 0
    with pytest.raises(ConvNetError, match="status -1"):
        net.grad_norm_of(buf[:6])
    with pytest.raises(ConvNetError, match="status -1"):
        net.grad_norm_of(buf[1:5])
    out = net.grad_norm_of(buf[4:12])
    net.synchronize()
    assert out.item() == np.float32(np.sqrt(8.0))


def test_state():
    import torch
    from mercer_research_amd.convnet import ConvNetError
    spec = FUSED_HEAD
    in_shape, layers, B = spec
    a, b = twins(spec, "fp32")
    sgd = (MU, WD, False)
    a.set_sgd(*sgd)
    a.set_ema(0.9)
    x, y = batch(a, spec)
    p = a.get_params()
    v, e = np.zeros_like(p), p.copy()
    gdev, gpad = grad(b, x, y)
    m1 = float(grad_norm(gpad) / np.float32(2))
    m2 = float(grad_norm(gpad) / np.float32(8))
    a.set_clip(m1)
    lr = 0.05
    for k in range(3):                                   # eager, replays
        step(a, x, y, lr)
        norm, coef = a.grad_norm()
        p, v, e, norm_ref = _host_step(b, x, y, p, v, e, lr, coef, sgd, 0.9)
        check_norm(f"m1 step {k}", norm, coef, norm_ref, m1)
    graphs = a.graphs_instantiated()
    # a changed max_norm between two replays reaches the next step: a new coefficient, the graphs dropped
    a.set_clip(m2)
    step(a, x, y, lr)
    norm, coef = a.grad_norm()
    p, v, e, norm_ref = _host_step(b, x, y, p, v, e, lr, coef, sgd, 0.9)
    check_norm("m2", norm, coef, norm_ref, m2)
    assert coef < 1.0 and a.graphs_instantiated() == graphs + 1
    assert same_bits(a.get_params(), p) and same_bits(a.get_velocity(), v) and same_bits(a.get_ema(), e)
    # refusals change nothing
    count = a.grad_norm_count()
    for bad in (float("nan"), -1.0, -INF):
        with pytest.raises(ConvNetError, match="status -1"):
            a.set_clip(bad)
        assert a.get_clip() == np.float32(m2)
    ring = torch.empty(4, dtype=torch.float32, device=a.device)
    with pytest.raises(ConvNetError, match="status -1"):                               # cap = 0 with a pointer: the library refuses
        a._ck(a.lib.rcn_hipx_set_grad_norm_log(a.net, ring.data_ptr(), 0))
    with pytest.raises(ValueError):                                                    # an empty tensor (its pointer is NULL): the wrapper
        a.set_grad_norm_log(torch.empty(0, dtype=torch.float32, device=a.device))
    assert a.grad_norm_count() == count == 4 and a.graphs_instantiated() == graphs + 1
    step(a, x, y, lr)                                   # (a replay: nothing was dropped by the refusals)
    norm, coef = a.grad_norm()
    p, v, e, norm_ref = _host_step(b, x, y, p, v, e, lr, coef, sgd, 0.9)
    assert a.graphs_instantiated() == graphs + 1 and same_bits(a.get_params(), p)
    # gradients() returns the raw gradient with clipping on, evaluate is unchanged
    b.set_params(p)
    _, ga = grad(a, x, y)
    _, gb = grad(b, x, y)
    assert np.array_equal(ga.view(np.uint32), gb.view(np.uint32))
    a0 = make_net(spec)
    a0.set_params(p)
    a0.set_clip(m1)
    assert np.array_equal(grad(a0, x, y)[1].view(np.uint32), gb.view(np.uint32))
    rng = np.random.default_rng(8)
    X = a.to_device(rng.integers(0, 256, (4 * B,) + in_shape).astype(np.uint8))
    Y = a.to_device(rng.integers(0, 10, 4 * B).astype(np.int32))
    a.synchronize()
    assert a.evaluate(X, Y) == b.evaluate(X, Y) and a.grad_norm_count() == 5
    # velocity, average and clip state survive set_params and set_precision
    before = (a.get_velocity(), a.get_ema(), a.grad_norm(), a.get_clip(), a.grad_norm_count())
    a.set_params(p)
    a.set_precision("bf16")
    a.set_precision("fp32")
    after = (a.get_velocity(), a.get_ema(), a.grad_norm(), a.get_clip(), a.grad_norm_count())
    assert same_bits(before[0], after[0]) and same_bits(before[1], after[1]) and before[2:] == after[2:]
    step(a, x, y, lr)
    norm, coef = a.grad_norm()
    p, v, e, norm_ref = _host_step(b, x, y, p, v, e, lr, coef, sgd, 0.9)
    check_norm("after set_params / set_precision", norm, coef, norm_ref, m2)
    assert same_bits(a.get_params(), p) and same_bits(a.get_velocity(), v) and same_bits(a.get_ema(), e)
    a.close(); b.close(); a0.close()
