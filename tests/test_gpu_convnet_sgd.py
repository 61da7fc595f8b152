"""GPU tests of the Track-X optimiser (include/rcn_hipx.h, rcn_hipx_set_sgd): SGD with momentum, weight decay and Nesterov fused into the
training step's one reduction launch (k_reduce_all_sgd), and its data-parallel half (k_sgd_apply).

The exactness tests run twin nets from the same parameters: net A trains with the fused step; net B computes the same gradients
(rcn_hipx_gradients_dev: the same kernels and sums as the step) and the update is applied on the host by tests/_sgd_ref.py, a float32
restatement with every operation rounded once.  The GPU update uses no fused multiply-add, so parameters and velocity agree bit for bit."""
import numpy as np
import pytest
from _convnet_util import CIFAR, FUSED_HEAD, MNIST, MU, PLAIN_HEAD, POOL_PAIRS, WD, batches, grad, make_net, step, twins
from _sgd_ref import sgd_update

from oracle import convnet_oracle as co

pytestmark = pytest.mark.gpu

def _host_step(twin, x, y, p, v, lr, mu, wd, nesterov):
    """The reference step: twin's gradients at p, then the float32 restatement of the update on the host."""
    twin.set_params(p)
    g = twin.unpad(grad(twin, x, y)[0])
    return sgd_update(p, g, v, lr, mu, wd, nesterov)


def _check_fused_against_host(spec, precision, nesterov, lrs):
    a, b = twins(spec, precision)
    a.set_sgd(MU, WD, nesterov)
    assert a.get_sgd() == (pytest.approx(MU), pytest.approx(WD), nesterov)
    plan = a.plan_of_this_net(spec[2])
    assert "k_reduce_all_sgd" in plan and "momentum 0.9" in plan and ("nesterov on" if nesterov else "nesterov off") in plan, plan
    x, y = batches(a, spec, 1)[0]
    p, v = a.get_params(), np.zeros(a.n_logical, dtype=np.float32)
    for k, lr in enumerate(lrs):
        step(a, x, y, lr)
        p, v = _host_step(b, x, y, p, v, lr, MU, WD, nesterov)
        pa, va = a.get_params(), a.get_velocity()
        assert np.array_equal(pa, p), (k, float(np.abs(pa - p).max()))
        assert np.array_equal(va, v), (k, float(np.abs(va - v).max()))
    assert np.abs(v).max() > 0
    a.close(); b.close()


def test_default_setting_is_plain_sgd_bit_for_bit():
    """(0, 0, False) given explicitly is a net never configured: the same kernels, the same bits, the same plan text."""
    a, b = twins(FUSED_HEAD, "fp32")
    a.set_sgd(0.0, 0.0, False)
    assert a.get_sgd() == (0.0, 0.0, False)
    assert a.plan_of_this_net(FUSED_HEAD[2]) == b.plan_of_this_net(FUSED_HEAD[2])
    assert "k_reduce_all_sgd" not in a.plan_of_this_net(FUSED_HEAD[2])
    p0 = a.get_params()
    xa, ya = batches(a, FUSED_HEAD, 1)[0]
    xb, yb = batches(b, FUSED_HEAD, 1)[0]
    for _ in range(4):                                   # eager, then graph replays
        step(a, xa, ya, 0.05)
        step(b, xb, yb, 0.05)
    assert np.array_equal(a.get_params(), b.get_params())
    assert not np.array_equal(a.get_params(), p0)
    assert np.array_equal(a.get_velocity(), np.zeros(a.n_logical, dtype=np.float32))
    a.close(); b.close()


@pytest.mark.parametrize("nesterov", [False, True])
@pytest.mark.parametrize("spec,precision", [(FUSED_HEAD, "fp32"), (PLAIN_HEAD, "fp32"), (FUSED_HEAD, "bf16"), (PLAIN_HEAD, "bf16"), (POOL_PAIRS, "bf16_stored")],
                         ids=["fused_head-fp32", "plain_head-fp32", "fused_head-bf16", "plain_head-bf16", "pool_pairs-bf16_stored"])
def test_fused_step_is_the_host_update_bit_for_bit(spec, precision, nesterov):
    """Five steps: eager, graph replays, one step at a second lr (a second graph), and back to the first graph."""
    _check_fused_against_host(spec, precision, nesterov, [0.05, 0.05, 0.05, 0.02, 0.05])


@pytest.mark.parametrize("spec", [FUSED_HEAD, PLAIN_HEAD], ids=["fused_head", "plain_head"])
def test_three_momentum_steps_match_the_f64_oracle_and_torch_sgd(spec):
    """Three steps with momentum 0.9 and weight decay 5e-4 against oracle.convnet_oracle's f64 gradients and torch.optim.SGD in float64,
    in the fp32 tolerance style of tests/test_gpu_convnet.py: |d| <= 6e-4 * scale + 1e-6."""
    import torch
    in_shape, layers, B = spec
    rng = np.random.default_rng(B)
    shapes = co.param_shapes(in_shape, layers)
    ws = [rng.standard_normal(k) * np.sqrt(2.0 / k[0]) for k, _ in shapes]
    bs = [rng.standard_normal(n) * 0.1 for _, n in shapes]
    flat = co.flatten(ws, bs).astype(np.float32)
    net = make_net(spec)
    net.set_params(flat)
    net.set_sgd(MU, WD, False)
    x = rng.standard_normal((B,) + in_shape).astype(np.float32)
    y = rng.integers(0, layers[-1][1], B).astype(np.int32)
    xd, yd = net.to_device(x), net.to_device(y)
    net.synchronize()
    lr = 0.05
    tp = torch.tensor(flat.astype(np.float64), requires_grad=True)
    opt = torch.optim.SGD([tp], lr=lr, momentum=MU, weight_decay=WD)
    for _ in range(3):
        w64, b64 = co.unflatten(tp.detach().numpy().copy(), in_shape, layers)
        _, _, gws, gbs = co.loss_and_grads(x.astype(np.float64), y, w64, b64, layers)
        tp.grad = torch.tensor(co.flatten(gws, gbs))
        opt.step()
        step(net, xd, yd, lr)
        ref, got = tp.detach().numpy(), net.get_params().astype(np.float64)
        scale = max(1e-3, float(np.abs(ref).max()))
        assert np.abs(got - ref).max() <= 6e-4 * scale + 1e-6, (float(np.abs(got - ref).max()), scale)
    buf = opt.state[tp]["momentum_buffer"].numpy()
    vscale = max(1e-3, float(np.abs(buf).max()))
    assert np.abs(net.get_velocity() - buf).max() <= 6e-4 * vscale + 1e-6
    net.close()


@pytest.mark.parametrize("precision", ["fp32", "bf16_stored"])
def test_data_parallel_half_is_the_fused_step_bit_for_bit(precision):
    """gradients_bucketed + apply_sgd(grad, 1, lr) == train_step over three steps, parameters and velocity; and apply_sgd(2 g, 0.5, lr) too.
    rcn_hipx_apply_dev stays the plain axpy and leaves the velocity alone."""
    import torch
    spec = POOL_PAIRS
    a, b = twins(spec, precision)
    c = make_net(spec, precision)
    c.set_params(a.get_params())
    for n in (a, b, c):
        n.set_sgd(MU, WD, True)
    x, y = batches(a, spec, 1)[0]
    grad = torch.empty(b.n_padded, dtype=torch.float32, device=b.device)
    lr = 0.03
    for _ in range(3):
        step(a, x, y, lr)
        with torch.cuda.stream(b.stream):
            b.gradients_bucketed(x, y, grad, None, 0)
            b.apply_sgd(grad, 1.0, lr)
        b.synchronize()
        with torch.cuda.stream(c.stream):
            c.gradients_bucketed(x, y, grad, None, 64 << 10)
            g2 = grad * 2.0
            c.apply_sgd(g2, 0.5, lr)
        c.synchronize()
        pa, va = a.get_params(), a.get_velocity()
        for n in (b, c):
            assert np.array_equal(n.get_params(), pa) and np.array_equal(n.get_velocity(), va)
    v_before = b.get_velocity()
    with torch.cuda.stream(b.stream):
        b.apply(grad, lr)
    b.synchronize()
    assert np.array_equal(b.get_velocity(), v_before)
    a.close(); b.close(); c.close()


def test_state_saved_and_loaded_continues_bit_for_bit_and_changes_reach_the_replay():
    import torch
    spec = FUSED_HEAD
    a, b = twins(spec, "fp32")
    three = batches(a, spec, 3, seed=4)
    lr = 0.05
    for n in (a, b):
        n.set_sgd(MU, WD, False)
    for k in range(6):
        step(a, *three[k % 3], lr)
    for k in range(3):
        step(b, *three[k % 3], lr)
    p3, v3 = b.get_params(), b.get_velocity()
    b.close()
    c = make_net(spec)
    assert np.array_equal(c.get_velocity(), np.zeros(c.n_logical, dtype=np.float32))       # no buffer yet: zeros
    with pytest.raises(Exception):
        c.set_velocity(v3)                               # momentum 0: -6
    c.set_params(p3)
    c.set_sgd(MU, WD, False)
    c.set_velocity(v3)
    for k in range(3, 6):
        step(c, *three[k % 3], lr)
    assert np.array_equal(c.get_params(), a.get_params()) and np.array_equal(c.get_velocity(), a.get_velocity())
    # the velocity survives set_params and a change of precision
    c.set_params(p3)
    c.set_precision("bf16")
    c.set_precision("fp32")
    assert np.array_equal(c.get_velocity(), a.get_velocity())

    # reset_velocity and a changed setting on a net whose step is already a captured graph: the next step sees them
    twin = make_net(spec)
    x, y = three[0]
    for _ in range(2):
        step(c, x, y, lr)                               # (the graph for (x, y, lr) exists and has been replayed)
    p = c.get_params()
    c.reset_velocity()
    step(c, x, y, lr)
    p, v = _host_step(twin, x, y, p, np.zeros(c.n_logical, dtype=np.float32), lr, MU, WD, False)
    assert np.array_equal(c.get_params(), p) and np.array_equal(c.get_velocity(), v)
    step(c, x, y, lr)                                   # replay after the reset
    p, v = _host_step(twin, x, y, p, v, lr, MU, WD, False)
    assert np.array_equal(c.get_params(), p) and np.array_equal(c.get_velocity(), v)
    c.set_sgd(0.5, 1e-3, True)
    assert c.get_sgd() == (0.5, pytest.approx(1e-3), True)
    step(c, x, y, lr)
    p, v = _host_step(twin, x, y, p, v, lr, 0.5, 1e-3, True)
    assert np.array_equal(c.get_params(), p) and np.array_equal(c.get_velocity(), v)
    # weight decay alone: the velocity is neither read nor written
    c.set_sgd(0.0, 1e-3, False)
    v_kept = c.get_velocity()
    step(c, x, y, lr)
    p, _ = _host_step(twin, x, y, p, v_kept, lr, 0.0, 1e-3, False)
    assert np.array_equal(c.get_params(), p) and np.array_equal(c.get_velocity(), v_kept)
    a.close(); c.close(); twin.close()


def test_invalid_settings_are_refused_and_change_nothing():
    from mercer_research_amd.convnet import ConvNetError
    net = make_net(FUSED_HEAD)
    net.set_sgd(0.5, 1e-4, True)
    for args in ((1.0, 0.0, False), (-0.1, 0.0, False), (float("nan"), 0.0, False), (0.9, -1e-4, False), (0.9, float("inf"), False), (0.0, 1e-4, True)):
        with pytest.raises(ConvNetError):
            net.set_sgd(*args)
        assert net.get_sgd() == (0.5, pytest.approx(1e-4), True)
    net.close()


@pytest.mark.parametrize("spec,precision", [(CIFAR, "fp32"), (MNIST, "bf16_stored")], ids=["cifar-b512-fp32", "mnist-b4096-bf16_stored"])
def test_fused_step_at_baseline_shapes(spec, precision):
    """The reduction's many-chunk and many-job paths at real sizes: two steps, bit for bit against the host update."""
    _check_fused_against_host(spec, precision, False, [0.02, 0.02])
