"""GPU tests of Track X's strided depthwise convolution and its batch-normalisation kinds without a ReLU (include/rcn_hipx.h:
RCN_HIPX_DWCONV3X3_S2, RCN_HIPX_BN, RCN_HIPX_BN_ADD; csrc/convnet_dw_s2.hpp: k_dw_s2_fwd, k_dw_s2_dgrad, k_dw_s2_wgrad; csrc/convnet_bn.hpp:
k_bn_apply) against PyTorch on the CPU in float64 (tests/_mb_ref.py) on the eight nets of that file, each in fp32 and bf16, net d once more
on a looping grid of three workgroups: tests/_twin_checks.py's schedule -- a gradients call, two plain SGD steps, a forward and an
evaluation on the running statistics -- compared quantity by quantity at the stride tests' bounds (fp32 2e-4 of a tensor's scale + 1e-6,
4e-4 after a second step; bf16 operands 5e-3 / 2e-2 against the twin with the same operand rounding, which leaves the depthwise layers
unrounded), no tensor widened.  Then a small-integer net whose logits are the same bits in both precisions and NumPy's integers; on net e
(two inverted residual blocks back to back and a strided one) twins, the second stream, the bucket walk, the epoch's one graph, save / load
and the three evaluation paths held bit for bit; one update per optimiser family against torch.optim; the bf16_stored refusal; create's
own refusals beside the plans'; rcn_hipx_step_flops by hand; and the benchmark's cifar_mbv2 description at a small batch."""
import functools

import numpy as np
import pytest
from _convnet_util import LR, batches, dev, epoch, make_net, same_bits, step, twins
from _mb_ref import BN, BNA, DWS2, LOOPING, M_A, M_D, M_E, M_S, NETS, OPTIONS, PW, RTOL, RTOL_2, STEPS, X_SPEC, MbNet, against_torch, case, compare, exact_case
from _twin_checks import device_run, grads, twin_schedule

pytestmark = pytest.mark.gpu

# (net, precision, the options of the device run): every net in both precisions; net d once more per precision on three looping workgroups
CASES = [(n, p, OPTIONS[n]) for n in sorted(NETS) for p in ("fp32", "bf16")] + [("d", p, LOOPING) for p in ("fp32", "bf16")]


@functools.lru_cache(maxsize=None)
def _reference(name, precision):
    """the twin's side of a case, once; nothing changes it"""
    spec = NETS[name]
    flat, x, y = case(name)
    return twin_schedule(MbNet(spec[0], spec[1], flat, operand="bf16" if precision == "bf16" else "f64"), x, y, STEPS)


@pytest.mark.parametrize("name,precision,options", CASES, ids=[f"{n}-{p}{'-looping' if o == LOOPING else ''}" for n, p, o in CASES])
def test_schedule_against_the_float64_twin(name, precision, options):
    spec = NETS[name]
    flat, x, y = case(name)
    r = device_run(spec, precision, flat, x, y, STEPS, options=tuple(options))
    compare(spec, r, _reference(name, precision), RTOL[precision], RTOL_2[precision], STEPS, f"net {name} {precision}{' looping' if options == LOOPING else ''}")


def test_step_flops_by_hand():
    """18 FLOP per OUTPUT element and pass of a strided depthwise layer: three passes, two as layer 0; beside the other layers' GEMMs"""
    net = make_net(M_A, "fp32")
    B = M_A[2]
    hand = 2 * 2 * 9 * (B * 4 * 6) * 3 * 32 + 3 * 2 * (B * 2 * 3) * 9 * 32 + 3 * 2 * B * 32 * 7
    assert net.step_flops(B) == hand, (net.step_flops(B), hand)
    net.close()
    net = make_net(M_D, "fp32")
    B = M_D[2]
    m1, m2 = B * 20 * 36, B * 10 * 18
    hand = 2 * 2 * m1 * 9 * 32 + 3 * 2 * m1 * 32 * 256 + 3 * 2 * m2 * 9 * 256 + 3 * 2 * B * 256 * 10
    assert net.step_flops(B) == hand, (net.step_flops(B), hand)
    net.close()


BR = (("bn_relu",),)
CREATE_REFUSALS = [
    # (input shape, layers, status, the message as every plan gives it: tests/test_convnet_mb_plan.py)
    ((4, 4, 3), ((DWS2,),) + BR + (("dense", 4),), -3, r"layer 0 \(RCN_HIPX_DWCONV3X3_S2\): .*multiple of 32, not 3"),
    ((6, 5, 32), ((DWS2,),) + BR + (("dense", 4),), -3, r"layer 0 \(RCN_HIPX_DWCONV3X3_S2\): .*even height and width, not 6x5"),
    ((4, 4, 32), ((DWS2,), ("conv", 32), ("dense", 4)), -2, r"layer 0 \(RCN_HIPX_DWCONV3X3_S2\): .*followed directly by a batch-normalisation layer"),
    ((4, 4, 3), (("conv", 32), (BN,), ("conv", 32), ("dense", 4)), -2, r"layer 1 \(RCN_HIPX_BN\): .*must directly follow a bias-only convolution"),
    ((4, 4, 3), (("conv_linear", 32), ("bn_relu",), (PW, 32), (BN,), ("global_avgpool",), ("dense", 4)), -2, r"layer 3 \(RCN_HIPX_BN\): .*without a ReLU must be followed directly by a convolution"),
    ((4, 4, 3), (("conv_linear", 32), ("bn_relu",), (PW, 32), (BNA, 2), ("pool",), ("dense", 4)), -2, r"layer 3 \(RCN_HIPX_BN_ADD\): .*without a ReLU must be followed directly by a convolution"),
    ((4, 4, 3), (("conv_linear", 32), ("bn_relu",), (PW, 32), (BNA, 1), ("conv", 32), ("dense", 4)), -1, r"layer 3 \(RCN_HIPX_BN_ADD\): .*at least 2, not 1"),
]


@pytest.mark.parametrize("in_shape,layers,status,message", CREATE_REFUSALS, ids=[str(k) for k in range(len(CREATE_REFUSALS))])
def test_create_refuses_as_the_plans_do(in_shape, layers, status, message):
    """rcn_hipx_create's own describe_layers path: the status and the message the plans give for the same description"""
    from mercer_research_amd import convnet
    from mercer_research_amd.convnet import ConvNet, ConvNetError
    with pytest.raises(ConvNetError, match=rf"{status}: {message}") as of_plan:
        convnet.plan(in_shape, layers, 2)
    with pytest.raises(ConvNetError, match=rf"{status}.*{message}") as of_create:
        ConvNet(in_shape, layers, 2)
    assert str(of_plan.value).split("layer ", 1)[1] == str(of_create.value).split("layer ", 1)[1], (str(of_plan.value), str(of_create.value))


# ---- exact data: the check that rests on no tolerance ---------------------------------------------------------------------------------------

def test_integer_net_gives_the_same_bits_in_both_precisions_and_numpy():
    import torch
    flat, stats, x, want, a1, a2 = exact_case()
    assert (a1 < 0).mean() > 0.2 and (a2 > 0).mean() > 0.2 and np.abs(want).max() < 2 ** 24 and len(np.unique(want)) > 10
    for precision in ("fp32", "bf16"):
        net = make_net(X_SPEC, precision)
        net.set_params(flat)
        net.set_bn_stats(stats)
        with torch.cuda.stream(net.stream):
            z = net.forward(dev(net, x))
        net.synchronize()
        z = z.cpu().numpy()
        net.close()
        assert same_bits(z, want.astype(np.float32)), (precision, np.abs(z - want).max())


# ---- held bit for bit on net e: two inverted residual blocks back to back, then a strided one ------------------------------------------------

def _state(net):
    return net.get_params(), net.get_bn_stats(), net.get_velocity()


def _same(a, b):
    return all(same_bits(u, v) for u, v in zip(a, b))


def _close(*nets):
    for n in nets:
        n.close()


def _twins(spec, precision, count, **kw):
    """_convnet_util.twins, and the plan's word that the kinds' kernels run"""
    nets = twins(spec, precision, count, **kw)
    for n in nets:
        text = n.plan_of_this_net(spec[2])
        assert "k_dw_s2_fwd" in text and "k_dw_s2_dgrad<3>" in text and "k_dw_s2_wgrad" in text and "k_bn_apply_add," in text and "k_bn_apply," in text and "linear: no gate" in text, text
    return nets


@pytest.mark.parametrize("precision", ["fp32", "bf16"])
def test_twins_are_bit_identical(precision):
    a, b = _twins(M_E, precision, 2, sgd=(0.9, 0.0, False))
    for x, y in batches(a, M_E, 3):
        step(a, x, y, LR)
        step(b, x, y, LR)
    assert _same(_state(a), _state(b)) and a.get_velocity().any()
    _close(a, b)


def test_overlap_changes_no_bit():
    """the weight gradients on the second stream read out[S] and dout[S + 1], never the dout[S] that the input gradient and the skip's add write"""
    a, b = _twins(M_E, "fp32", 2)
    b.set_overlap(1)
    x, y = batches(a, M_E, 1)[0]
    ga, la, za = grads(a, x, y, M_E[2])
    gb, lb, zb = grads(b, x, y, M_E[2])
    assert same_bits(ga, gb) and la == lb and same_bits(za, zb)
    for _ in range(2):
        step(a, x, y, LR)
        step(b, x, y, LR)
    assert _same(_state(a), _state(b))
    _close(a, b)


@pytest.mark.parametrize("min_bytes", [0, 4000])
def test_buckets_that_cut_inside_a_block_change_no_bit(min_bytes):
    """at 0 bytes every layer is a bucket: one ends between a skip's add and its source, and between the two blocks whose sums chain; at
    4000 bytes a bucket edge lies inside a block"""
    import torch
    net, = _twins(M_E, "fp32", 1)
    x, y = batches(net, M_E, 1)[0]
    g, _, _ = grads(net, x, y, M_E[2])
    gb = torch.zeros(net.n_padded, dtype=torch.float32, device=net.device)
    seen = []
    with torch.cuda.stream(net.stream):
        net.gradients_bucketed(x, y, gb, min_bucket_bytes=min_bytes, on_bucket=lambda *a: seen.append(a))
    net.synchronize()
    assert len(seen) > 2 and same_bits(net.unpad(gb), g)
    net.close()


def test_epoch_equals_steps():
    in_shape, layers, B = M_E
    a, b = _twins(M_E, "fp32", 2)
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


def test_save_and_load_rebuild_the_kinds_and_continue_bit_for_bit(tmp_path):
    """the state stores the distance of a bn_add and the resolved width of a depthwise layer; the loaded net is the same net, running
    statistics of the linear layers included"""
    from mercer_research_amd.convnet import ConvNet
    a, = _twins(M_E, "fp32", 1, sgd=(0.9, 5e-4, True))
    bs = batches(a, M_E, 4)
    for x, y in bs[:2]:
        step(a, x, y, LR)
    a.save(tmp_path / "mb.state", extra=b"loop state")
    b, extra = ConvNet.load(tmp_path / "mb.state", M_E[2])
    resolved = [(l[0], 64) if l[0] in ("dwconv_linear", DWS2) else tuple(l) for l in M_E[1]]
    assert extra == b"loop state" and b.layers == resolved and b.layers[7] == (BNA, 6) and b.layers[19] == (BN,)
    assert _same(_state(a), _state(b))
    for x, y in bs[2:]:
        step(a, x, y, LR)
        step(b, x, y, LR)
    assert _same(_state(a), _state(b))
    _close(a, b)


def test_evaluate_metrics_evaluate_and_forward_agree():
    import torch
    net, = _twins(M_E, "fp32", 1)
    x, y = batches(net, M_E, 1)[0]
    step(net, x, y, LR)
    with torch.cuda.stream(net.stream):
        z = net.forward(x)
    net.synchronize()
    z = z.cpu().numpy()
    loss, correct = net.evaluate(x, y, x_scale=1.0, x_shift=0.0)
    rep = net.evaluate_metrics(x, y, topk=(1,), confusion=False, logits=True, x_scale=1.0, x_shift=0.0)
    assert same_bits(rep.logits, z) and rep.correct == correct == int((z.argmax(1) == y.cpu().numpy()).sum()) and rep.loss == loss
    net.close()


# ---- the recipe, refusals, the benchmark's description --------------------------------------------------------------------------------------

def test_sgd_momentum_nesterov_step_against_torch():
    import torch
    against_torch(M_E, lambda n: n.set_sgd(0.9, 5e-4, True), lambda p: (torch.optim.SGD(p, lr=LR, momentum=0.9, weight_decay=5e-4, nesterov=True), LR, None), tag="SGD momentum nesterov")


def test_adamw_step_against_torch():
    """eps = 1e-4 for the reason tests/test_gpu_convnet_bn_recipe.py gives: a convolution's bias in front of batch normalisation has gradient
    zero in exact arithmetic, and Adam would turn fp32 rounding noise there into steps."""
    import torch
    lr, wd = 1e-2, 0.05
    against_torch(M_E, lambda n: n.set_adam((0.9, 0.999), 1e-4, wd, True), lambda p: (torch.optim.AdamW(p, lr=lr, betas=(0.9, 0.999), eps=1e-4, weight_decay=wd), lr, None), tag="AdamW")


def test_clip_accumulate_two_and_ema_against_torch():
    import torch

    def configure(n):
        n.set_clip(0.25)
        n.set_accumulate(2)
    against_torch(M_E, configure, lambda p: (torch.optim.SGD(p, lr=LR), LR, 0.25), micro=2, tag="clip 0.25 + accumulate 2 + EMA 0.9", ema=0.9)


def test_bf16_stored_is_refused_and_changes_nothing():
    """through the batch-normalisation rule, as for RCN_HIPX_CONV3X3"""
    from mercer_research_amd.convnet import ConvNetError
    net, = twins(M_S, "fp32", 1)
    x, y = batches(net, M_S, 1)[0]
    before = net.plan_of_this_net(M_S[2])
    with pytest.raises(ConvNetError, match=r"-3: .*batch normalisation"):
        net.set_precision("bf16_stored")
    assert net.plan_of_this_net(M_S[2]) == before and "fp32 operands" in before and "k_dw_s2_dgrad<0>" in before
    step(net, x, y, LR)
    net.close()


def test_cifar_mbv2_description_trains_at_a_small_batch():
    """bench_convnet.py's cifar_mbv2 at B = 8: create accepts its 31 layers with parameters and the loss falls over a few steps"""
    import torch
    import bench_convnet
    in_shape, layers, _ = bench_convnet.CONFIGS["cifar_mbv2"]
    assert sum(l[0] not in ("pool", "global_avgpool") for l in layers) == 31
    net = make_net((in_shape, layers, 8), "fp32")
    net.init_params(1)
    rng = np.random.default_rng(0)
    x, y = dev(net, rng.standard_normal((8,) + in_shape).astype(np.float32)), dev(net, rng.integers(0, 10, 8).astype(np.int32))
    loss = torch.zeros(1, dtype=torch.float32, device=net.device)
    seen = []
    for _ in range(6):
        step(net, x, y, 0.02, loss)
        seen.append(float(loss.item()))
    print("cifar_mbv2 at B = 8, loss per step:", [round(s, 4) for s in seen])
    assert np.isfinite(seen).all() and seen[-1] < seen[0], seen
    net.close()
