"""GPU tests of Track X's batch normalisation (include/rcn_hipx.h: RCN_HIPX_CONV3X3, RCN_HIPX_BN_RELU; csrc/convnet_bn.hpp) against PyTorch
on the CPU in float64 (tests/_torch_ref.py): the logits of a training forward, the loss, the gradients per tensor, the parameters and the
running statistics after two steps, and the forward / evaluation on the running statistics afterwards, on the four nets of
tests/test_convnet_bn_plan.py -- the smallest at which each path (pool-gated, gated by the convolution above, self-gated, many partials
per channel) can go wrong.

Tolerances: fp32 against f64 is the project's 2e-4 of a tensor's scale + 1e-6, 4e-4 after a second step
(tests/test_gpu_convnet.py).  bf16 operands are held to the forms tests' bound, 5e-3 (2e-2 after two steps), against the float64 twin with
the SAME operand rounding (TorchNet(operand="bf16"): the convolutions' and dense layers' operands rounded to bf16 in all three GEMMs,
batch normalisation in float64), as those tests hold them to the oracle with the rounding mirrored; the training logits also to
tests/test_gpu_convnet.py's 3e-2 against the unrounded twin.  (Rounding the operands alone moves a gradient tensor of net a by up to
8 % of its scale in float64 torch itself -- invstd and the two mean subtractions amplify -- so the unrounded twin says nothing at 5e-3.)"""
import numpy as np
import pytest
from _convnet_util import LR, close, dev, make_net, same_bits, step, sync
from _torch_ref import TorchNet, close_per_tensor, random_params, tensor_slices
from test_convnet_bn_plan import BN_B, BN_C, BN_NETS

pytestmark = pytest.mark.gpu

RTOL = {"fp32": 2e-4, "bf16": 5e-3}
RTOL_2 = {"fp32": 4e-4, "bf16": 2e-2}                   # after a second step
CASES = [("a", "fp32"), ("a", "bf16"), ("b", "fp32"), ("c", "fp32"), ("d", "fp32")]


def _data(spec, seed=3):
    in_shape, layers, B = spec
    rng = np.random.default_rng(seed)
    flat = random_params(rng, in_shape, layers)
    x = rng.standard_normal((B,) + in_shape).astype(np.float32)
    y = rng.integers(0, layers[-1][1], B).astype(np.int32)
    return flat, x, y


def _run(spec, precision, flat, x, y, bn=None, steps=2):
    """What the device and the float64 twin make of: one gradients call (a training forward: the statistics advance), `steps` plain SGD
    steps, then a forward and an evaluation on the running statistics."""
    import torch
    in_shape, layers, B = spec
    net = make_net(spec, precision)
    ref = TorchNet(in_shape, layers, flat, *(bn or (0.1, 1e-5)), operand="bf16" if precision == "bf16" else "f64")
    if bn:
        net.set_bn(*bn)
    net.set_params(flat)
    xd, yd = dev(net, x), dev(net, y)
    out = {}
    loss = torch.zeros(1, dtype=torch.float32, device=net.device)
    with torch.cuda.stream(net.stream):
        g = net.gradients(xd, yd, loss=loss)
        z = net.last_logits(B)
    net.synchronize()
    out["grad"] = net.unpad(g)
    out["loss"], out["logits"], out["stats1"] = float(loss.item()), z.cpu().numpy(), net.get_bn_stats()
    out["ref_loss"], out["ref_logits"], out["ref_grad"] = ref.loss_and_grads(x, y)
    out["ref_stats1"] = ref.bn_stats().copy()
    losses = []
    for _ in range(steps):
        step(net, xd, yd, LR, loss)
        losses.append(float(loss.item()))
    out["losses"], out["ref_losses"] = losses, [ref.sgd_step(x, y, LR) for _ in range(steps)]
    out["params"], out["stats"], out["ref_params"], out["ref_stats"] = net.get_params(), net.get_bn_stats(), ref.params(), ref.bn_stats().copy()
    with torch.cuda.stream(net.stream):
        ze = net.forward(xd)
    net.synchronize()
    out["eval_logits"], out["ref_eval_logits"] = ze.cpu().numpy(), ref.logits(x, train=False)
    out["eval"] = net.evaluate(xd, yd, x_scale=1.0, x_shift=0.0)
    zr = out["ref_eval_logits"]
    lse = np.log(np.exp(zr - zr.max(1, keepdims=True)).sum(1)) + zr.max(1)
    out["ref_eval"] = (float((lse - zr[np.arange(B), y]).mean()), int((zr.argmax(1) == y).sum()))
    out["margin"] = float(np.min(np.sort(zr, axis=1)[:, -1] - np.sort(zr, axis=1)[:, -2]))
    net.close()
    return out


@pytest.fixture(scope="module", params=CASES, ids=[f"{n}-{p}" for n, p in CASES])
def case(request):
    name, precision = request.param
    spec = BN_NETS[name]
    return name, precision, spec, _run(spec, precision, *_data(spec))


def test_training_forward_logits_and_loss(case):
    name, precision, spec, r = case
    close(r["logits"], r["ref_logits"], RTOL[precision], f"{name} {precision} training logits")
    close([r["loss"]], [r["ref_loss"]], RTOL[precision], f"{name} {precision} loss")
    if precision == "bf16":
        flat, x, y = _data(spec)
        close(r["logits"], TorchNet(spec[0], spec[1], flat).logits(x, train=True), 3e-2, f"{name} bf16 training logits against the unrounded twin")


def test_gradients_per_tensor(case):
    name, precision, spec, r = case
    assert np.isfinite(r["grad"]).all()
    close_per_tensor(r["grad"], r["ref_grad"], spec[0], spec[1], RTOL[precision], f"{name} {precision} gradient")


def test_running_statistics_after_one_training_forward(case):
    name, precision, spec, r = case
    close(r["stats1"], r["ref_stats1"], RTOL[precision], f"{name} {precision} running statistics after gradients()")
    assert np.abs(r["stats1"] - r["stats"]).max() > 1e-3          # ... and they went on moving with the two steps


def test_parameters_and_statistics_after_two_steps(case):
    name, precision, spec, r = case
    for got, ref in zip(r["losses"], r["ref_losses"]):
        close([got], [ref], RTOL_2[precision], f"{name} {precision} step loss")
    close_per_tensor(r["params"], r["ref_params"], spec[0], spec[1], RTOL_2[precision], f"{name} {precision} parameters")
    close(r["stats"], r["ref_stats"], RTOL_2[precision], f"{name} {precision} running statistics after two steps")


def test_forward_and_evaluate_use_the_running_statistics(case):
    name, precision, spec, r = case
    close(r["eval_logits"], r["ref_eval_logits"], RTOL_2[precision], f"{name} {precision} evaluation logits")
    # the evaluation logits are NOT the training forward's: the running statistics are three momentum steps from (0, 1), not the batch's
    assert np.abs(r["eval_logits"] - r["logits"]).max() > 10 * RTOL_2[precision] * np.abs(r["ref_eval_logits"]).max()
    (loss, correct), (rloss, rcorrect) = r["eval"], r["ref_eval"]
    close([loss], [rloss], RTOL_2[precision], f"{name} {precision} evaluation loss")
    scale = float(np.abs(r["ref_eval_logits"]).max())
    if r["margin"] > 4 * RTOL_2[precision] * scale:       # no row's two best logits are within reach of the tolerance: the count is exact
        assert correct == rcorrect, (correct, rcorrect)


# ---- more cases ---------------------------------------------------------------------------------------------------------------------------

def test_constant_channel_is_finite_and_has_zero_gamma_gradient():
    """Channel 0's convolution weights are zero, so x = bias over the whole batch: variance 0.  Finite everywhere, xh = 0, so
    y = max(0, beta) and d gamma = 0 -- exactly -- and everything still equals torch, which sees the same degenerate channel."""
    import torch
    spec = BN_C
    in_shape, layers, B = spec
    flat, x, y = _data(spec, seed=5)
    (w0, b0), (g1, be1), (wd, bd) = tensor_slices(in_shape, layers)
    W = flat[w0].reshape(27, 32); W[:, 0] = 0.0; W[:, 1] = 0.0
    flat[b0][0], flat[b0][1] = 0.75, -0.5
    flat[be1][0], flat[be1][1] = 0.5, -0.25              # y = 0.5 in channel 0 and 0 in channel 1, everywhere
    net = make_net(spec, "fp32")
    net.set_params(flat)
    xd, yd = dev(net, x), dev(net, y)
    with torch.cuda.stream(net.stream):
        g = net.gradients(xd, yd)
        z = net.last_logits(B)
    net.synchronize()
    gl, z = net.unpad(g), z.cpu().numpy()
    assert np.isfinite(gl).all() and np.isfinite(z).all() and np.isfinite(net.get_bn_stats()).all()
    assert gl[g1][0] == 0.0 and gl[g1][1] == 0.0, gl[g1][:2]
    ref = TorchNet(in_shape, layers, flat)
    _, rz, rg = ref.loss_and_grads(x, y)
    close(z, rz, 2e-4, "constant channel: training logits")
    # y = max(0, beta) whatever gamma is: the logits do not move by a bit when the constant channels' gamma does
    flat2 = flat.copy(); flat2[g1][0], flat2[g1][1] = 3.0, -2.0
    net.set_params(flat2)
    with torch.cuda.stream(net.stream):
        net.gradients(xd, yd)
        z2 = net.last_logits(B)
    net.synchronize()
    assert same_bits(z2.cpu().numpy(), z)
    # channel 1's gate is shut (y = 0): nothing flows into its beta; channel 0's beta gets the whole gradient
    assert gl[be1][1] == 0.0 and gl[be1][0] != 0.0
    # Channel 0's dx is gamma * invstd * (g - mean g) with invstd = 1 / sqrt(eps) = 316: large, and torch's too.  The convolution's BIAS
    # gradient is the sum of dx over the rows, which is zero in exact arithmetic (the mean is subtracted): float64 leaves 1e-17 there
    # and the device the rounding of a sum of 32 terms of channel 0's size, 4e-6 -- no value to be relative to.  It is a sum of the
    # same dZ terms as the layer's weight gradient (inputs of unit variance), so it is held at THAT tensor's scale.  This is a deliberate
    # loosening of the per-tensor rule for this one tensor, argued from the arithmetic -- not a measured 10x bound.
    close_per_tensor(gl, rg, in_shape, layers, 2e-4, "constant channel: gradient", bias_at_weight_scale=(0,))
    stats = net.get_bn_stats()
    assert stats[0] != 0.0 and abs(stats[32] - 0.81) < 1e-6          # two forwards: mean moved, var = 0.9^2 * 1 + momentum * 0
    net.close()


def test_set_bn_non_default_values_against_torch():
    spec = BN_B
    r = _run(spec, "fp32", *_data(spec, seed=7), bn=(0.3, 1e-3))
    close(r["logits"], r["ref_logits"], 2e-4, "set_bn: training logits")
    close_per_tensor(r["grad"], r["ref_grad"], spec[0], spec[1], 2e-4, "set_bn: gradient")
    close(r["stats"], r["ref_stats"], 4e-4, "set_bn: running statistics")
    close_per_tensor(r["params"], r["ref_params"], spec[0], spec[1], 4e-4, "set_bn: parameters")
    close(r["eval_logits"], r["ref_eval_logits"], 4e-4, "set_bn: evaluation logits")
    # ... and they differ from the defaults' run: the values reached the kernels
    d = _run(spec, "fp32", *_data(spec, seed=7))
    assert np.abs(d["stats"] - r["stats"]).max() > 1e-3 and np.abs(d["logits"] - r["logits"]).max() > 1e-5


def test_set_bn_refusals_and_getters():
    from mercer_research_amd.convnet import ConvNetError
    net = make_net(BN_C, "fp32")
    assert net.get_bn() == (np.float32(0.1), np.float32(1e-5), 1)
    for bad in ((-0.1, 1e-5), (1.5, 1e-5), (0.1, 0.0), (float("nan"), 1e-5), (0.1, float("inf"))):
        with pytest.raises(ConvNetError, match="status -1"):
            net.set_bn(*bad)
    net.set_bn(1.0, 1e-3)
    assert net.get_bn()[:2] == (1.0, np.float32(1e-3))
    s = net.get_bn_stats()
    assert s.size == 64 and np.array_equal(s, np.r_[np.zeros(32), np.ones(32)].astype(np.float32))
    net.set_bn_stats(np.arange(64, dtype=np.float32))
    assert np.array_equal(net.get_bn_stats(), np.arange(64, dtype=np.float32))
    net.reset_bn_stats()
    assert np.array_equal(net.get_bn_stats(), s)
    with pytest.raises(ConvNetError, match="status -3.*batch normalisation"):
        net.set_precision("bf16_stored")
    net.close()
    plain = make_net(((4, 4, 3), (("conv", 32), ("dense", 6)), 2), "fp32")
    plain.set_bn()                                        # the defaults: accepted, nothing to do
    with pytest.raises(ConvNetError, match="status -3"):
        plain.set_bn(0.2, 1e-5)
    assert plain.get_bn_stats().size == 0
    plain.close()


def test_fewer_than_two_rows_is_refused_before_anything_is_enqueued():
    """B * H * W = 1: the unbiased variance has no value.  -2, and neither the parameters, the statistics nor the graph count move."""
    import torch
    from mercer_research_amd.convnet import ConvNetError
    spec = ((1, 1, 3), (("conv_linear", 32), ("bn_relu",), ("dense_relu", 32), ("dense", 4)), 2)
    net = make_net(spec, "fp32")
    net.init_params(1)
    net.set_dropout(0.5, 7)                               # (a refused step must not tick the dropout ordinal either)
    p0, s0 = net.get_params(), net.get_bn_stats()
    x, y = dev(net, np.ones((1, 1, 1, 3), dtype=np.float32)), dev(net, np.zeros(1, dtype=np.int32))
    with torch.cuda.stream(net.stream):
        with pytest.raises(ConvNetError, match="status -2.*two rows"):
            net.train_step(x, y, LR)
        with pytest.raises(ConvNetError, match="status -2.*two rows"):
            net.gradients(x, y)
    sync()
    assert same_bits(net.get_params(), p0) and same_bits(net.get_bn_stats(), s0) and net.graphs_instantiated() == 0
    assert net.dropout_state() == 0
    net.set_precision("bf16")                             # (... nor make the operand copies)
    with torch.cuda.stream(net.stream):
        with pytest.raises(ConvNetError, match="status -2.*two rows"):
            net.train_step(x, y, LR)
    sync()
    assert net.dropout_state() == 0 and same_bits(net.get_bn_stats(), s0)
    net.close()


def test_a_batch_below_max_batch_that_needs_more_partials():
    """A 32 x 32 map with max_batch = 33: the largest batch has 33792 rows = 264 partials of 128 rows, a batch of 32 has 32768 rows = 512
    partials of 64 rows (tests/test_convnet_bn_plan.py holds the arithmetic).  The layer's buffer, sized once, must hold them: the step
    equals float64 torch, and the same net built with max_batch = 32 bit for bit -- the sums depend on the batch, not on max_batch."""
    import torch
    from mercer_research_amd.convnet import ConvNetError, bn_partials
    spec = ((32, 32, 3), (("conv_linear", 32), ("bn_relu",), ("pool",), ("dense", 10)), 32)
    in_shape, layers, B = spec
    assert bn_partials(32 * 1024)[0] > bn_partials(33 * 1024)[0]
    flat, x, y = _data(spec, seed=9)
    out = []
    for max_batch in (33, 32):
        net = make_net(spec, "fp32", max_batch=max_batch)
        net.set_params(flat)
        xd, yd = dev(net, x), dev(net, y)
        with torch.cuda.stream(net.stream):
            with pytest.raises(ConvNetError, match="status -6.*no forward pass"):
                net.last_logits(B)
            g = net.gradients(xd, yd)
            z = net.last_logits(B)
            with pytest.raises(ConvNetError, match="status -6.*another batch size"):
                net.last_logits(B - 1)
        net.synchronize()
        gl, z = net.unpad(g), z.cpu().numpy()
        step(net, xd, yd, LR)
        step(net, xd, yd, LR)                             # (the replayed graph)
        out.append((gl, z, net.get_params(), net.get_bn_stats()))
        net.close()
    assert all(same_bits(u, v) for u, v in zip(*out))
    ref = TorchNet(in_shape, layers, flat)
    _, rz, rg = ref.loss_and_grads(x, y)
    close(out[0][1], rz, 2e-4, "B < max_batch: training logits")
    close_per_tensor(out[0][0], rg, in_shape, layers, 2e-4, "B < max_batch: gradient")
    ref.sgd_step(x, y, LR)
    ref.sgd_step(x, y, LR)
    close_per_tensor(out[0][2], ref.params(), in_shape, layers, 4e-4, "B < max_batch: parameters after two steps")
    close(out[0][3], ref.bn_stats(), 4e-4, "B < max_batch: running statistics")
