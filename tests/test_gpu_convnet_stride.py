"""GPU tests of Track X's two downsampling layer kinds (include/rcn_hipx.h: RCN_HIPX_CONV3X3_S2, RCN_HIPX_BN_ADD_RELU_DOWN; csrc/convnet.hpp:
k_conv_fwd / k_conv_wgrad on ConvShapeS2 and the parity-class input gradient on ConvShapeS2T; csrc/convnet_bn.hpp: k_bn_apply_relu with a
SkipDown, k_skip_bwd_add_down) against PyTorch on the CPU in float64 (tests/_stride_ref.py) on the nets of that file: tests/_twin_checks.py's
schedule -- a gradients call, two plain SGD steps, a forward and an evaluation on the running statistics -- compared quantity by quantity
at the residual tests' bounds (fp32 2e-4 of a tensor's scale + 1e-6, 4e-4 after a second step; bf16 operands 5e-3 / 2e-2 against the twin
with the same operand rounding), no tensor widened; then twins held bit for bit, the identity check of the shortcut, one update per
optimiser family against torch.optim, and the benchmark's cifar_resnet14 description at 8 x 8 x 3.

The worst share of an allowance per case, from a run on an MI355X, is in profiles/trackx_stride_tests.txt."""
import numpy as np
import pytest
from _convnet_util import LR, batches, dev, epoch, make_net, same_bits, step, twins
from _stride_ref import D_A, D_B, NETS, OPTIONS, RTOL, RTOL_2, STEPS, StrideNet, against_torch, case, layout, layout_spec, resnet14
from _torch_ref import random_params, tensor_slices
from _twin_checks import compare, device_run, grads, twin_schedule

pytestmark = pytest.mark.gpu

# (net, precision, options of the device run): every net in both precisions; net a once more with the weight gradient's narrowing policies
# off, which is where the 64-wide strided weight-gradient forms run (tests/test_convnet_stride_plan.py: every form is reached)
NO_POLICY = (("wgf_policy", 0), ("wgb_policy", 0))
CASES = [(n, p, OPTIONS[n]) for n in sorted(NETS) for p in ("fp32", "bf16")] + [("a", "fp32", NO_POLICY), ("a", "bf16", NO_POLICY)]


@pytest.mark.parametrize("name,precision,options", CASES, ids=[f"{n}-{p}{'-nopolicy' if o == NO_POLICY else ''}" for n, p, o in CASES])
def test_schedule_against_the_float64_twin(name, precision, options):
    spec = NETS[name]
    flat, x, y = case(name)
    ref = twin_schedule(StrideNet(spec[0], spec[1], flat, operand="bf16" if precision == "bf16" else "f64"), x, y, STEPS)
    r = device_run(spec, precision, flat, x, y, STEPS, options=options)
    compare(layout_spec(spec), r, ref, RTOL[precision], RTOL_2[precision], STEPS, f"net {name} {precision}{' no policy' if options == NO_POLICY else ''}")


def test_resnet14_description_at_8x8(tmp_path):
    """bench_convnet.py's cifar_resnet14 at 8 x 8 x 3, B = 3: 27 reduction jobs and a state pack that carry both kinds"""
    spec = resnet14((8, 8, 3), 3)
    in_shape, layers, B = spec
    flat = random_params(np.random.default_rng(3), in_shape, layout(layers))
    rng = np.random.default_rng(4)
    x, y = rng.standard_normal((B,) + in_shape).astype(np.float32), rng.integers(0, 10, B).astype(np.int32)
    # (fp32, the deep tests' practice: at 2 x 2 x 3 = 12 rows per channel in the last stage the bf16 twin measures its own rounding flips)
    ref = twin_schedule(StrideNet(in_shape, layers, flat), x, y, STEPS)
    compare(layout_spec(spec), device_run(spec, "fp32", flat, x, y, STEPS), ref, RTOL["fp32"], RTOL_2["fp32"], STEPS, "resnet14 at 8x8 fp32")
    from mercer_research_amd.convnet import ConvNet
    a = make_net(spec, "fp32", sgd=(0.9, 5e-4, True))
    a.set_params(flat)
    step(a, dev(a, x), dev(a, y), LR)
    a.save(tmp_path / "r14.state")
    b, _ = ConvNet.load(tmp_path / "r14.state", B)
    assert b.layers == [tuple(l) for l in layers] and _same(_state(a), _state(b))
    _close(a, b)


def test_step_flops_of_one_strided_layer():
    """3 GEMMs x 2 x 9 x M_out x Cin x Cout for the strided layer (layer 1: it has an input gradient), by hand beside the other layers'"""
    in_shape, layers, B = D_A
    net = make_net(D_A, "fp32")
    m_in, m_out = B * 4 * 12, B * 2 * 6
    hand = 2 * 2 * 9 * m_in * 3 * 32 + 3 * 2 * 9 * m_out * 32 * 64 + 3 * 2 * 9 * m_out * 64 * 64 + 3 * 2 * B * 64 * 7
    assert net.step_flops(B) == hand, (net.step_flops(B), hand)
    net.close()


# ---- twins held bit for bit (net b: both kinds twice, sources a bn_add_relu and a bn_add_relu_down) -----------------------------------------

def _state(net):
    return net.get_params(), net.get_bn_stats(), net.get_velocity()


def _same(a, b):
    return all(same_bits(u, v) for u, v in zip(a, b))


def _close(*nets):
    for n in nets:
        n.close()


@pytest.mark.parametrize("precision", ["fp32", "bf16"])
def test_twins_are_bit_identical(precision):
    a, b = twins(D_B, precision, 2, sgd=(0.9, 0.0, False))
    for x, y in batches(a, D_B, 3):
        step(a, x, y, LR)
        step(b, x, y, LR)
    assert _same(_state(a), _state(b)) and a.get_velocity().any()
    _close(a, b)


def test_overlap_changes_no_bit():
    """the weight gradients on the second stream read out[S] and dout[S + 1], never the dout[S] the parity launch and the strided add write"""
    a, b = twins(D_B, "fp32", 2)
    b.set_overlap(1)
    x, y = batches(a, D_B, 1)[0]
    ga, la, za = grads(a, x, y, D_B[2])
    gb, lb, zb = grads(b, x, y, D_B[2])
    assert same_bits(ga, gb) and la == lb and same_bits(za, zb)
    for _ in range(2):
        step(a, x, y, LR)
        step(b, x, y, LR)
    assert _same(_state(a), _state(b))
    _close(a, b)


@pytest.mark.parametrize("min_bytes", [0, 80000])
def test_buckets_that_cut_inside_a_down_block_change_no_bit(min_bytes):
    """at 0 bytes every layer is a bucket: one ends between the strided add (in the iteration of layer S + 1, the strided convolution) and
    layer S"""
    import torch
    net, = twins(D_B, "fp32", 1)
    x, y = batches(net, D_B, 1)[0]
    g, _, _ = grads(net, x, y, D_B[2])
    gb = torch.zeros(net.n_padded, dtype=torch.float32, device=net.device)
    seen = []
    with torch.cuda.stream(net.stream):
        net.gradients_bucketed(x, y, gb, min_bucket_bytes=min_bytes, on_bucket=lambda *a: seen.append(a))
    net.synchronize()
    assert len(seen) > 2 and same_bits(net.unpad(gb), g)
    net.close()


def test_epoch_equals_steps():
    in_shape, layers, B = D_B
    a, b = twins(D_B, "fp32", 2)
    rng = np.random.default_rng(2)
    n = 3 * B
    X, y = rng.standard_normal((n,) + in_shape).astype(np.float32), rng.integers(0, 10, n).astype(np.int32)
    perm = rng.permutation(n).astype(np.int32)
    epoch(a, dev(a, X), dev(a, y), dev(a, perm), B, LR)
    for s in range(3):
        rows = perm[s * B:(s + 1) * B]
        step(b, dev(b, X[rows]), dev(b, y[rows]), LR)
    assert _same(_state(a), _state(b)) and a.graphs_instantiated() == 1
    _close(a, b)


def test_save_and_load_rebuild_both_kinds_and_continue_bit_for_bit(tmp_path):
    from mercer_research_amd.convnet import ConvNet
    a, = twins(D_B, "fp32", 1, sgd=(0.9, 5e-4, True))
    bs = batches(a, D_B, 4)
    for x, y in bs[:2]:
        step(a, x, y, LR)
    a.save(tmp_path / "down.state", extra=b"loop state")
    b, extra = ConvNet.load(tmp_path / "down.state", D_B[2])
    assert extra == b"loop state" and b.layers == [tuple(l) for l in D_B[1]] and b.layers[6] == ("conv_linear_s2", 64) and b.layers[9] == ("bn_add_relu_down", 4)
    assert _same(_state(a), _state(b))
    for x, y in bs[2:]:
        step(a, x, y, LR)
        step(b, x, y, LR)
    assert _same(_state(a), _state(b))
    _close(a, b)


def test_evaluate_metrics_evaluate_and_forward_agree():
    import torch
    net, = twins(D_B, "fp32", 1)
    x, y = batches(net, D_B, 1)[0]
    step(net, x, y, LR)
    with torch.cuda.stream(net.stream):
        z = net.forward(x)
    net.synchronize()
    z = z.cpu().numpy()
    loss, correct = net.evaluate(x, y, x_scale=1.0, x_shift=0.0)
    rep = net.evaluate_metrics(x, y, topk=(1,), confusion=False, logits=True, x_scale=1.0, x_shift=0.0)
    assert same_bits(rep.logits, z) and rep.correct == correct == int((z.argmax(1) == y.cpu().numpy()).sum()) and rep.loss == loss
    net.close()


# ---- the shortcut alone ---------------------------------------------------------------------------------------------------------------------

def test_down_block_with_zero_gamma_and_beta_is_the_shortcut():
    """Net a with gamma = beta = 0 in the down block's second batch normalisation: y = max(0, fl(fl(fl(xh * 0) + 0) + s')) = s' for the
    non-negative source (a ReLU output), bit for bit.  The source map comes from the device itself, through the truncated net `conv 32,
    dense 1536` whose dense layer is the identity (every logit is one element times 1 plus exact zeros: the map's own bits); NumPy
    subsamples and pads it, and takes the mean over 2 x 6 and the dense layer in float64: the logits agree at the fp32 bound.  That the
    block's output is s' and nothing else is then held bit for bit: with the main path's two convolutions re-drawn, no logit bit moves."""
    import torch
    from _convnet_util import close
    in_shape, layers, B = D_A
    flat, x, y = case("a")
    sl = tensor_slices(in_shape, layout(layers))              # conv 0, strided conv 1, bn 2, conv 3, bn 4 (down), dense 5
    flat = flat.copy()
    flat[sl[4][0]] = 0.0
    flat[sl[4][1]] = 0.0

    def logits_of(spec, p):
        net = make_net(spec, "fp32")
        net.set_params(p)
        with torch.cuda.stream(net.stream):
            z = net.forward(dev(net, x))
        net.synchronize()
        z = z.cpu().numpy()
        net.close()
        return z
    z = logits_of(D_A, flat)
    K = 4 * 12 * 32
    reader = np.concatenate([flat[sl[0][0]], flat[sl[0][1]], np.eye(K, dtype=np.float32).ravel(), np.zeros(K, dtype=np.float32)])
    s = logits_of((in_shape, (("conv", 32), ("dense", K)), B), reader).reshape(B, 4, 12, 32)
    assert (s >= 0).all() and (s > 0).mean() > 0.2
    sp = np.zeros((B, 2, 6, 64))
    sp[..., 16:48] = s[:, ::2, ::2, :]
    want = sp.mean((1, 2)) @ flat[sl[5][0]].reshape(64, 7).astype(np.float64) + flat[sl[5][1]]
    close(z, want, 2e-4, "zero gamma and beta: logits against the NumPy shortcut of the device's source map")
    flat2 = flat.copy()
    rng = np.random.default_rng(9)
    for t in (sl[1][0], sl[3][0]):
        flat2[t] = (rng.standard_normal(flat2[t].size) * 0.05).astype(np.float32)
    assert same_bits(logits_of(D_A, flat2), z), "the block's output depends on its main path although gamma = beta = 0"


# ---- the recipe -----------------------------------------------------------------------------------------------------------------------------

def test_sgd_momentum_nesterov_step_against_torch():
    import torch
    against_torch(D_A, lambda n: n.set_sgd(0.9, 5e-4, True), lambda p: (torch.optim.SGD(p, lr=LR, momentum=0.9, weight_decay=5e-4, nesterov=True), LR, None), tag="SGD momentum nesterov")


def test_adamw_step_against_torch():
    """eps = 1e-4 for the reason tests/test_gpu_convnet_bn_recipe.py gives: a convolution's bias in front of batch normalisation has gradient
    zero in exact arithmetic, and Adam would turn fp32 rounding noise there into steps."""
    import torch
    lr, wd = 1e-2, 0.05
    against_torch(D_A, lambda n: n.set_adam((0.9, 0.999), 1e-4, wd, True), lambda p: (torch.optim.AdamW(p, lr=lr, betas=(0.9, 0.999), eps=1e-4, weight_decay=wd), lr, None), tag="AdamW")


def test_clip_and_accumulate_two_against_torch():
    import torch

    def configure(n):
        n.set_clip(0.25)
        n.set_accumulate(2)
    against_torch(D_A, configure, lambda p: (torch.optim.SGD(p, lr=LR), LR, 0.25), micro=2, tag="clip 0.25 + accumulate 2")
