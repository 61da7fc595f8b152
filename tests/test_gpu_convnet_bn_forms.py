"""GPU tests of batch normalisation at the workload's shapes and kernel forms (cases: tests/_bn_cases.py; tests/test_convnet_bn_forms_plan.py
proves on the CPU that each case reaches what it names, and that the exact reference has teeth):
  A  FORMS: epilogue 1 (bias only) of the LDS-tiled convolution kernels, their epilogue-3 input gradients gated by a BN layer's output,
     and partials of 128 rows, against tests/_torch_ref.TorchNet in float64 -- with the operands rounded to bf16 where "bf16" precision
     rounds them: training logits and loss, the gradient per tensor, parameters per tensor and running statistics after two plain SGD
     steps, evaluation logits on the running statistics.
  B  the looping forms of those kernels on grids of 1, 2, 3, 5 and 7 workgroups ("halo_f32_slots"): bit for bit the one-item-per-workgroup
     run, running statistics included; the pipelined bf16 kernel bit for bit its unpipelined twin.
  C  SHAPES: the statistics kernels at every (M, C) where they take another path, on data whose convolution output is exact: the running
     statistics after one training forward within ONE float32 ulp of the float64 host formula in every channel.  (One, not none: the
     device may contract var = q / M - mean * mean into a fused multiply-add.)  A tolerance cannot see one row of 33792; this can.
  D  host paths that had not met a BN net: gradient buckets, label smoothing, the pair step.
Tolerances are the project's (tests/test_gpu_convnet_bn.py): fp32 against float64 2e-4 of a tensor's scale + 1e-6, 4e-4 after a second
step; bf16 operands against the twin with the same rounding 5e-3, 2e-2 after two steps.  Everything is held at its own scale but ONE kind
of tensor, as tests/test_gpu_convnet_bn.py::test_constant_channel_is_finite_and_has_zero_gamma_gradient argues: the GRADIENT of a
convolution's bias in front of a BN layer is the sum over the rows of dx, zero in exact arithmetic (the mean is subtracted) -- it has no
scale of its own, and what the device leaves there is the rounding of a sum of up to 33792 terms of dZ, the terms of the same layer's
weight gradient.  It is held at that tensor's scale (close_per_tensor's bias_at_weight_scale)."""
import functools
from types import SimpleNamespace

import numpy as np
import pytest
from _bn_cases import BF16P_TWIN_LINES, BN_EPS, BN_MOMENTUM, FORMS, LOOPING, SHAPES, conv_linear_layers, conv_output, exact_data, host_stats, rows_of, shape_id, shape_spec
from _convnet_util import close, dev, make_net, same_bits, zeros
from _forms_cases import SLOTS, names
from _oracle_steps import LR
from _torch_ref import TorchNet, close_per_tensor, random_params
from test_convnet_bn_plan import BN_A

pytestmark = pytest.mark.gpu

RTOL = {"fp32": 2e-4, "bf16": 5e-3}
RTOL_2 = {"fp32": 4e-4, "bf16": 2e-2}                   # after a second step
# The step rate of the two steps is tests/_oracle_steps.py's, for its reason: these nets put the logits layer straight on thousands of
# features, and at tests/_convnet_util.py's 0.05 the first step overshoots into a saturated softmax (the twin's loss on bn-r128: 3.6, then 89)
BIT_KEYS = ("logits", "loss", "grad", "stats1", "params1", "params2", "stats2", "loss2", "eval_logits")


def frozen(ns):
    for a in vars(ns).values():
        if isinstance(a, np.ndarray):
            a.setflags(write=False)
    return ns


@functools.lru_cache(maxsize=None)
def reference(spec, precision):
    """Parameters, one batch and the float64 twin's results in `precision`'s mode, once per (net, mode): one training forward and
    backward, two plain SGD steps, then the evaluation forward.  The arrays are read-only."""
    in_shape, layers, B = spec
    rng = np.random.default_rng(B + in_shape[0])
    flat = random_params(rng, in_shape, layers)
    x = rng.standard_normal((B,) + in_shape).astype(np.float32)
    y = rng.integers(0, layers[-1][1], B).astype(np.int32)
    twin = TorchNet(in_shape, layers, flat, operand="bf16" if precision == "bf16" else "f64")
    loss, logits, grad = twin.loss_and_grads(x, y)
    stats1 = twin.bn_stats().copy()
    loss1 = twin.sgd_step(x, y, LR)
    params1 = twin.params()
    loss2 = twin.sgd_step(x, y, LR)
    return frozen(SimpleNamespace(spec=spec, flat=flat, x=x, y=y, loss=loss, logits=logits, grad=grad, stats1=stats1, loss1=loss1, params1=params1, loss2=loss2,
                                  params2=twin.params(), stats2=twin.bn_stats().copy(), eval_logits=twin.logits(x, train=False)))


def setup(case):
    """the case's net with its options set (its plan names the promised forms), its reference, its batch on the device"""
    ref = reference(case.spec, case.precision)
    net = make_net(case.spec, precision=None, tiling=case.tiling)
    for name, value in case.options.items():
        net.set_option(name, value)
    net.set_precision(case.precision)
    L = net.plan_of_this_net(case.spec[2]).splitlines()
    for text in case.lines:
        assert any(names(l, text) for l in L), (text, L)
    return net, ref, dev(net, ref.x.copy()), dev(net, ref.y.copy())


def run(net, ref, xd, yd):
    """from the reference's parameters and reset statistics: one gradients call (a training forward: the statistics advance), two training
    steps (the first eager, the second a replayed graph), then the forward on the running statistics"""
    import torch
    B = ref.spec[2]
    net.set_params(ref.flat)
    net.reset_bn_stats()
    loss = zeros(net, 1)
    with torch.cuda.stream(net.stream):
        g = net.gradients(xd, yd, loss=loss)
        z = net.last_logits(B)
    net.synchronize()
    out = {"logits": z.cpu().numpy(), "loss": loss.cpu().numpy(), "grad": g.cpu().numpy(), "grad_logical": net.unpad(g), "stats1": net.get_bn_stats()}
    for k in (1, 2):
        with torch.cuda.stream(net.stream):
            net.train_step(xd, yd, LR, loss)
        net.synchronize()
        out[f"params{k}"], out[f"loss{k}"] = net.get_params(), loss.cpu().numpy()       # loss{k}: the loss BEFORE update k
    out["stats2"] = net.get_bn_stats()
    with torch.cuda.stream(net.stream):
        ze = net.forward(xd)
    net.synchronize()
    out["eval_logits"] = ze.cpu().numpy()
    return out


def check_torch(out, ref, precision, tag):
    """returns the worst share of an allowance"""
    in_shape, layers, _ = ref.spec
    rtol, rtol2 = RTOL[precision], RTOL_2[precision]
    cl = conv_linear_layers(layers)
    assert all(np.isfinite(out[k]).all() for k in BIT_KEYS)
    used = [close(out["logits"], ref.logits, rtol, f"{tag} training logits"),
            close(out["loss"], [ref.loss], rtol, f"{tag} loss"),
            close_per_tensor(out["grad_logical"], ref.grad, in_shape, layers, rtol, f"{tag} gradient", bias_at_weight_scale=cl),
            close(out["stats1"], ref.stats1, rtol, f"{tag} running statistics after gradients()"),
            close(out["loss1"], [ref.loss1], rtol, f"{tag} loss before the first update"),
            # one step: the parameters (exact) minus LR times a gradient within rtol
            close_per_tensor(out["params1"], ref.params1, in_shape, layers, rtol, f"{tag} parameters after one step"),
            # ... and so is that step's displacement, a few thousandths of the parameters' scale at this rate (tests/_oracle_steps.py)
            close(out["params1"] - ref.flat.astype(np.float64), ref.params1 - ref.flat, rtol, f"{tag} displacement of the first step"),
            close(out["loss2"], [ref.loss2], rtol2, f"{tag} loss before the second update"),
            close_per_tensor(out["params2"], ref.params2, in_shape, layers, rtol2, f"{tag} parameters after two steps"),
            close(out["stats2"], ref.stats2, rtol2, f"{tag} running statistics after two steps"),
            close(out["eval_logits"], ref.eval_logits, rtol2, f"{tag} evaluation logits")]
    # the statistics moved with every training forward, and the evaluation logits are not the training forward's
    assert np.abs(out["stats1"] - out["stats2"]).max() > 1e-3
    assert np.abs(out["eval_logits"] - out["logits"]).max() > 10 * rtol2 * np.abs(ref.eval_logits).max()
    print(f"{tag}: worst share of an allowance = {max(used):.3f}")
    return max(used)


def assert_same_bits(tag, got, want):
    for k in BIT_KEYS:
        assert same_bits(got[k], want[k]), (tag, k, float(np.abs(got[k].astype(np.float64) - want[k]).max()), int((got[k] != want[k]).sum()))


# ---- A, B: the forms -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", FORMS, ids=[c.id for c in FORMS])
def test_forms_match_torch(case):
    """The bias gradient of every conv_linear layer is held at its layer's weight-gradient scale (the module's docstring says why);
    everything else at its own."""
    net, ref, xd, yd = setup(case)
    check_torch(run(net, ref, xd, yd), ref, case.precision, case.id)
    net.close()


@pytest.mark.parametrize("case", LOOPING, ids=[c.id for c in LOOPING])
def test_looping_changes_nothing_but_the_schedule(case):
    net, ref, xd, yd = setup(case)
    net.set_option("halo_f32_slots", 0)               # the grid is the items
    base = run(net, ref, xd, yd)
    plan = net.plan_of_this_net(case.spec[2])
    for s in SLOTS:
        net.set_option("halo_f32_slots", s)
        assert net.plan_of_this_net(case.spec[2]) == plan
        assert_same_bits(f"{s} workgroups", run(net, ref, xd, yd), base)
    net.close()


def test_the_pipelined_bf16_kernel_is_its_unpipelined_twin_bit_for_bit():
    case = next(c for c in FORMS if c.id == "bn-r128-bf16p")
    net, ref, xd, yd = setup(case)
    out = run(net, ref, xd, yd)
    for name, value in case.twin.items():
        net.set_option(name, value)
    L = net.plan_of_this_net(case.spec[2]).splitlines()
    for text in BF16P_TWIN_LINES:
        assert any(names(l, text) for l in L), (text, L)
    twin = run(net, ref, xd, yd)
    assert_same_bits(f"twin {case.twin}", twin, out)
    check_torch(twin, ref, case.precision, "bn-r128 unpipelined twin")
    net.close()


# ---- C: exact statistics -----------------------------------------------------------------------------------------------------------------------
def _exact_run(s, flat, v, y):
    import torch
    spec = shape_spec(s)
    net = make_net(spec, "fp32")
    net.set_bn(BN_MOMENTUM, BN_EPS)
    net.set_params(flat)
    xd, yd = dev(net, v), dev(net, y)
    with torch.cuda.stream(net.stream):
        g = net.gradients(xd, yd)
        z = net.last_logits(spec[2])
    net.synchronize()
    out = (net.get_bn_stats(), z.cpu().numpy(), net.unpad(g))
    net.close()
    return out


@pytest.mark.parametrize("s", SHAPES, ids=[shape_id(s) for s in SHAPES])
def test_statistics_are_exact_to_one_ulp(s):
    """x[m, c] = w_c v[m] + b_c is exact in float32 and its sums in double, so the running statistics after one training forward from
    (0, 1) at momentum 0.5 -- 0.5 mean and 0.5 + 0.5 var M / (M - 1) -- are the float64 host values to one float32 ulp in every channel
    (tests/test_convnet_bn_forms_plan.py: the host values round to the exact rational ones, and one row lost or doubled moves every channel
    by hundreds of ulps).  The logits, and at M <= 129 -- where one row is at least 0.8 % of a sum -- the gradient per tensor, against
    float64 torch at 2e-4; the convolution's bias gradient at its weight gradient's scale (the module's docstring)."""
    in_shape, layers, B = shape_spec(s)
    flat, v, y = exact_data(s)
    M, C = rows_of(s), s.C
    stats, z, g = _exact_run(s, flat, v, y)
    want = host_stats(conv_output(s, v))
    assert stats.dtype == np.float32 and stats.shape == want.shape == (2 * C,)
    ulps = np.abs(stats.astype(np.float64) - want) / np.spacing(np.abs(want).astype(np.float32)).astype(np.float64)
    print(f"{shape_id(s)} M = {M}: running mean off by at most {ulps[:C].max():.3f} ulps, running variance by {ulps[C:].max():.3f}; "
          f"{int((stats == want.astype(np.float32)).sum())} of {2 * C} values are the host's own float32")
    assert np.isfinite(stats).all() and ulps.max() <= 1.0, (int(ulps.argmax()), float(ulps.max()), stats[ulps.argmax()], want[ulps.argmax()])
    twin = TorchNet(in_shape, layers, flat, BN_MOMENTUM, BN_EPS)
    _, rz, rg = twin.loss_and_grads(v, y)
    close(z, rz, 2e-4, f"{shape_id(s)} training logits")
    if M <= 129:
        close_per_tensor(g, rg, in_shape, layers, 2e-4, f"{shape_id(s)} gradient", bias_at_weight_scale=conv_linear_layers(layers))
    # a second identical net gives the same bits: every sum has one order per shape
    again = _exact_run(s, flat, v, y)
    assert all(same_bits(a, b) for a, b in zip(again, (stats, z, g)))


# ---- D: host paths that carry a BN layer as they carry any layer ---------------------------------------------------------------------------------
def _bn_a(seed):
    in_shape, layers, B = BN_A
    rng = np.random.default_rng(seed)
    flat = random_params(rng, in_shape, layers)
    x = rng.standard_normal((B,) + in_shape).astype(np.float32)
    y = rng.integers(0, layers[-1][1], B).astype(np.int32)
    return in_shape, layers, B, flat, x, y, rng


def test_gradient_buckets_of_a_bn_net_are_the_plain_gradients():
    import torch
    in_shape, layers, B, flat, x, y, _ = _bn_a(11)
    net = make_net(BN_A, "fp32")
    net.set_params(flat)
    xd, yd = dev(net, x), dev(net, y)
    loss, loss2 = zeros(net, 1), zeros(net, 1)
    with torch.cuda.stream(net.stream):
        g = net.gradients(xd, yd, loss=loss)
    net.synchronize()
    s1 = net.get_bn_stats()
    for min_bytes in (0, 1 << 20):                        # one bucket per layer with parameters; everything in one bucket
        net.reset_bn_stats()
        g2 = torch.full_like(g, float("nan"))
        seen = []
        with torch.cuda.stream(net.stream):
            net.gradients_bucketed(xd, yd, g2, loss=loss2, min_bucket_bytes=min_bytes, on_bucket=lambda piece, k, n: seen.append((k, n, piece.numel())))
        net.synchronize()
        assert same_bits(g2.cpu().numpy(), g.cpu().numpy()) and same_bits(loss2.cpu().numpy(), loss.cpu().numpy()), min_bytes
        assert same_bits(net.get_bn_stats(), s1)          # one training forward each
        assert len(seen) == seen[0][1] and (len(seen) >= 6 if min_bytes == 0 else len(seen) == 1), seen
    close_per_tensor(net.unpad(g), TorchNet(in_shape, layers, flat).loss_and_grads(x, y)[2], in_shape, layers, 2e-4, "BN_A bucketed gradient")
    net.close()


def test_label_smoothing_on_a_bn_net_matches_torch():
    import torch
    in_shape, layers, B, flat, x, y, _ = _bn_a(12)
    net = make_net(BN_A, "fp32")
    net.set_loss(0.1)
    net.set_params(flat)
    xd, yd = dev(net, x), dev(net, y)
    loss = zeros(net, 1)
    with torch.cuda.stream(net.stream):
        g = net.gradients(xd, yd, loss=loss)
    net.synchronize()
    rloss, _, rg = TorchNet(in_shape, layers, flat).loss_and_grads(x, y, label_smoothing=0.1)
    hard, _, hg = TorchNet(in_shape, layers, flat).loss_and_grads(x, y)
    assert abs(rloss - hard) > 1e-2 and np.abs(rg - hg).max() > 1e-3        # (the smoothing is visible at the tolerance)
    close(loss.cpu().numpy(), [rloss], 2e-4, "BN_A smoothed loss")
    close_per_tensor(net.unpad(g), rg, in_shape, layers, 2e-4, "BN_A smoothed gradient")
    net.close()


def test_pair_step_on_a_bn_net_matches_torch():
    """target 0.3 onehot(ya) + 0.7 onehot(yb): the loss is the same blend of the two cross-entropies"""
    import torch
    in_shape, layers, B, flat, x, ya, rng = _bn_a(13)
    yb = ((ya + 1 + rng.integers(0, layers[-1][1] - 1, B)) % layers[-1][1]).astype(np.int32)      # never ya's class
    lr, wf = 0.05, float(np.float32(0.3))
    net = make_net(BN_A, "fp32")
    net.set_params(flat)
    xd, yad, ybd = dev(net, x), dev(net, ya), dev(net, yb)
    w = dev(net, np.array([0.3], dtype=np.float32))
    loss = zeros(net, 1)
    with torch.cuda.stream(net.stream):
        net.train_step_pair(xd, yad, ybd, w, lr, loss)
    net.synchronize()
    twin = TorchNet(in_shape, layers, flat)
    ce = torch.nn.functional.cross_entropy
    z = twin.forward(x, True)
    rloss = wf * ce(z, torch.from_numpy(ya.astype(np.int64))) + (1.0 - wf) * ce(z, torch.from_numpy(yb.astype(np.int64)))
    rloss.backward()
    with torch.no_grad():
        for p in twin.parameters():
            p -= lr * p.grad
    plain = TorchNet(in_shape, layers, flat)
    plain.sgd_step(x, ya, lr)
    assert np.abs(plain.params() - twin.params()).max() > 1e-3               # (the second labels are visible at the tolerance)
    close(loss.cpu().numpy(), [float(rloss.detach())], 2e-4, "BN_A pair loss")
    close_per_tensor(net.get_params(), twin.params(), in_shape, layers, 2e-4, "BN_A parameters after one pair step")
    close(net.get_bn_stats(), twin.bn_stats(), 2e-4, "BN_A running statistics after one pair step")
    net.close()
