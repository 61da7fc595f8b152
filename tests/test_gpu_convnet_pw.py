"""GPU tests of Track X's 1x1 convolution (include/rcn_hipx.h: RCN_HIPX_CONV1X1; csrc/convnet_pw.hpp: k_pw, the streaming kernel of its
forward pass and input gradient; csrc/convnet_select.hpp: select_pw, option "pw") against PyTorch on the CPU in float64 (tests/_pw_ref.py)
on the four nets of that file, each in fp32 and bf16 with the streaming kernel (pw = 1) and with the implicit-GEMM form (pw = 0):
tests/_twin_checks.py's schedule -- a gradients call, two plain SGD steps, a forward and an evaluation on the running statistics -- compared
quantity by quantity at the stride tests' bounds (fp32 2e-4 of a tensor's scale + 1e-6, 4e-4 after a second step; bf16 operands 5e-3 /
2e-2 against the twin with the same operand rounding), no tensor widened.  Then twins held bit for bit, a small-integer net whose logits
are the same bits from both forms, both precisions and NumPy's integers, one update per optimiser family against torch.optim, the
bf16_stored refusal, create's own refusals beside the plans', and the benchmark's cifar_bottleneck description at a small batch.  Every
test that is not about one form runs in both: the option "pw" defaults to the implicit GEMM, so a test that left it alone would never
launch k_pw (`_twins` sets it and asserts, by the net's own plan, that the form is the one the test names)."""
import functools

import numpy as np
import pytest
from _convnet_util import LR, batches, dev, epoch, make_net, same_bits, step, twins
from _pw_ref import LOOPING, NETS, OPTIONS, P_A, P_B, P_C, RTOL, RTOL_2, STEPS, X_SPEC, PwNet, against_torch, case, compare, exact_case
from _twin_checks import device_run, grads, twin_schedule

pytestmark = pytest.mark.gpu

# (net, precision, pw, the other options of the device run): every net in both precisions and both forms; net d once more per precision on
# three looping workgroups per column slice (sixteen row blocks: a workgroup takes five or six)
CASES = [(n, p, pw, OPTIONS[n]) for n in sorted(NETS) for p in ("fp32", "bf16") for pw in (1, 0)] + [("d", p, 1, LOOPING) for p in ("fp32", "bf16")]


@functools.lru_cache(maxsize=None)
def _reference(name, precision):
    """the twin's side of a case, once for both forms; nothing changes it"""
    spec = NETS[name]
    flat, x, y = case(name)
    return twin_schedule(PwNet(spec[0], spec[1], flat, operand="bf16" if precision == "bf16" else "f64"), x, y, STEPS)


@pytest.mark.parametrize("name,precision,pw,options", CASES, ids=[f"{n}-{p}-pw{w}{'-looping' if o == LOOPING else ''}" for n, p, w, o in CASES])
def test_schedule_against_the_float64_twin(name, precision, pw, options):
    spec = NETS[name]
    flat, x, y = case(name)
    r = device_run(spec, precision, flat, x, y, STEPS, options=tuple(options) + (("pw", pw),))
    compare(spec, r, _reference(name, precision), RTOL[precision], RTOL_2[precision], STEPS, f"net {name} {precision} pw {pw}{' looping' if options == LOOPING else ''}")


def test_step_flops_of_the_1x1_layers():
    """3 GEMMs x 2 x M x Cin x Cout per 1x1 layer (two GEMMs for layer 0), by hand beside the other layers'"""
    in_shape, layers, B = P_A
    net = make_net(P_A, "fp32")
    m = B * 4 * 6
    hand = 2 * 2 * 9 * m * 3 * 32 + 3 * 2 * m * 32 * 64 + 3 * 2 * B * 64 * 7
    assert net.step_flops(B) == hand, (net.step_flops(B), hand)
    net.close()


def test_step_flops_of_the_bottleneck_net():
    """net b: its first layer (two GEMMs), the block's two 1x1 layers and its 3x3 layer (three GEMMs each), the logits layer"""
    in_shape, layers, B = P_B
    net = make_net(P_B, "fp32")
    m = B * 6 * 10
    hand = 2 * 2 * 9 * m * 3 * 128 + 3 * 2 * m * 128 * 32 + 3 * 2 * 9 * m * 32 * 32 + 3 * 2 * m * 32 * 128 + 3 * 2 * B * 128 * 10
    assert net.step_flops(B) == hand, (net.step_flops(B), hand)
    net.close()


CREATE_REFUSALS = [
    # (input shape, layers, status, the message as every plan gives it: tests/test_convnet_pw_plan.py)
    ((4, 4, 3), (("conv1x1_linear", 32), ("bn_relu",), ("dense", 4)), -3, r"layer 0 \(RCN_HIPX_CONV1X1\): .*multiple of 32, not 3"),
    ((4, 4, 32), (("conv1x1_linear", 48), ("bn_relu",), ("dense", 4)), -3, r"layer 0 \(RCN_HIPX_CONV1X1\): .*positive multiple of 32"),
    ((4, 4, 32), (("dense_relu", 32), ("conv1x1_linear", 32), ("bn_relu",), ("dense", 4)), -2, r"layer 1 \(RCN_HIPX_CONV1X1\): .*after a dense layer or a global average pool"),
    ((4, 4, 32), (("conv1x1_linear", 32), ("conv", 32), ("dense", 4)), -2, r"layer 0 \(RCN_HIPX_CONV1X1\): .*followed directly by a batch-normalisation layer"),
    ((4, 4, 32), (("conv", 32), ("conv1x1_linear", 32)), -2, r"layer 1 \(RCN_HIPX_CONV1X1\): .*followed directly by a batch-normalisation layer"),
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

def test_integer_net_gives_the_same_bits_from_both_forms_both_precisions_and_numpy():
    import torch
    flat, stats, x, want, a2 = exact_case()
    assert (a2 > 0).mean() > 0.2 and np.abs(want).max() < 2 ** 24 and len(np.unique(want)) > 10
    for precision in ("fp32", "bf16"):
        for pw in (1, 0):
            net = make_net(X_SPEC, precision)
            net.set_option("pw", pw)
            net.set_params(flat)
            net.set_bn_stats(stats)
            with torch.cuda.stream(net.stream):
                z = net.forward(dev(net, x))
            net.synchronize()
            z = z.cpu().numpy()
            net.close()
            assert same_bits(z, want.astype(np.float32)), (precision, pw, np.abs(z - want).max())


# ---- twins held bit for bit (net b: the bottleneck block) -----------------------------------------------------------------------------------

def _state(net):
    return net.get_params(), net.get_bn_stats(), net.get_velocity()


def _same(a, b):
    return all(same_bits(u, v) for u, v in zip(a, b))


def _close(*nets):
    for n in nets:
        n.close()


def _twins(spec, precision, count, pw, **kw):
    """_convnet_util.twins with the form of the 1x1 layers set on every net: 1 = k_pw, 0 = the implicit GEMM (the option's default)"""
    nets = twins(spec, precision, count, **kw)
    for n in nets:
        n.set_option("pw", pw)
        assert f"k_pw<{'bf16' if precision == 'bf16' else 'f32'}, " in n.plan_of_this_net(spec[2]) if pw else "k_pw<" not in n.plan_of_this_net(spec[2]), "the net does not run the form the test is about"
    return nets

FORMS = pytest.mark.parametrize("pw", [1, 0], ids=["k_pw", "implicit-gemm"])


@pytest.mark.parametrize("pw", [1, 0])
@pytest.mark.parametrize("precision", ["fp32", "bf16"])
def test_twins_are_bit_identical(precision, pw):
    a, b = _twins(P_B, precision, 2, pw, sgd=(0.9, 0.0, False))
    for x, y in batches(a, P_B, 3):
        step(a, x, y, LR)
        step(b, x, y, LR)
    assert _same(_state(a), _state(b)) and a.get_velocity().any()
    _close(a, b)


@FORMS
def test_overlap_changes_no_bit(pw):
    """the weight gradients on the second stream read out[S] and dout[S + 1], never the dout[S] that the 1x1 layer's input-gradient launch
    (k_pw with pw = 1, the implicit GEMM with pw = 0) and the skip's add write"""
    a, b = _twins(P_B, "fp32", 2, pw)
    b.set_overlap(1)
    x, y = batches(a, P_B, 1)[0]
    ga, la, za = grads(a, x, y, P_B[2])
    gb, lb, zb = grads(b, x, y, P_B[2])
    assert same_bits(ga, gb) and la == lb and same_bits(za, zb)
    for _ in range(2):
        step(a, x, y, LR)
        step(b, x, y, LR)
    assert _same(_state(a), _state(b))
    _close(a, b)


@FORMS
@pytest.mark.parametrize("min_bytes", [0, 20000])
def test_buckets_that_cut_inside_a_bottleneck_change_no_bit(min_bytes, pw):
    """at 0 bytes every layer is a bucket: one ends between the skip's add (in the iteration of the block's first 1x1 layer) and the source"""
    import torch
    net, = _twins(P_B, "fp32", 1, pw)
    x, y = batches(net, P_B, 1)[0]
    g, _, _ = grads(net, x, y, P_B[2])
    gb = torch.zeros(net.n_padded, dtype=torch.float32, device=net.device)
    seen = []
    with torch.cuda.stream(net.stream):
        net.gradients_bucketed(x, y, gb, min_bucket_bytes=min_bytes, on_bucket=lambda *a: seen.append(a))
    net.synchronize()
    assert len(seen) > 2 and same_bits(net.unpad(gb), g)
    net.close()


@FORMS
def test_epoch_equals_steps(pw):
    in_shape, layers, B = P_B
    a, b = _twins(P_B, "fp32", 2, pw)
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


@FORMS
def test_save_and_load_rebuild_the_kind_and_continue_bit_for_bit(tmp_path, pw):
    """(the option is the net's, not the state's: the loaded net is given the same form)"""
    from mercer_research_amd.convnet import ConvNet
    a, = _twins(P_B, "fp32", 1, pw, sgd=(0.9, 5e-4, True))
    bs = batches(a, P_B, 4)
    for x, y in bs[:2]:
        step(a, x, y, LR)
    a.save(tmp_path / "pw.state", extra=b"loop state")
    b, extra = ConvNet.load(tmp_path / "pw.state", P_B[2])
    b.set_option("pw", pw)
    assert extra == b"loop state" and b.layers == [tuple(l) for l in P_B[1]] and b.layers[2] == ("conv1x1_linear", 32) and b.layers[6] == ("conv1x1_linear", 128)
    assert _same(_state(a), _state(b))
    for x, y in bs[2:]:
        step(a, x, y, LR)
        step(b, x, y, LR)
    assert _same(_state(a), _state(b))
    _close(a, b)


@FORMS
def test_evaluate_metrics_evaluate_and_forward_agree(pw):
    import torch
    net, = _twins(P_B, "fp32", 1, pw)
    x, y = batches(net, P_B, 1)[0]
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

def _with_form(pw, configure):
    def both(n):
        n.set_option("pw", pw)
        configure(n)
    return both


@FORMS
def test_sgd_momentum_nesterov_step_against_torch(pw):
    import torch
    against_torch(P_B, _with_form(pw, lambda n: n.set_sgd(0.9, 5e-4, True)), lambda p: (torch.optim.SGD(p, lr=LR, momentum=0.9, weight_decay=5e-4, nesterov=True), LR, None), tag="SGD momentum nesterov")


@FORMS
def test_adamw_step_against_torch(pw):
    """eps = 1e-4 for the reason tests/test_gpu_convnet_bn_recipe.py gives: a convolution's bias in front of batch normalisation has gradient
    zero in exact arithmetic, and Adam would turn fp32 rounding noise there into steps."""
    import torch
    lr, wd = 1e-2, 0.05
    against_torch(P_B, _with_form(pw, lambda n: n.set_adam((0.9, 0.999), 1e-4, wd, True)), lambda p: (torch.optim.AdamW(p, lr=lr, betas=(0.9, 0.999), eps=1e-4, weight_decay=wd), lr, None), tag="AdamW")


@FORMS
def test_clip_accumulate_two_and_ema_against_torch(pw):
    import torch

    def configure(n):
        n.set_clip(0.25)
        n.set_accumulate(2)
    against_torch(P_B, _with_form(pw, configure), lambda p: (torch.optim.SGD(p, lr=LR), LR, 0.25), micro=2, tag="clip 0.25 + accumulate 2 + EMA 0.9", ema=0.9)


def test_bf16_stored_is_refused_and_changes_nothing():
    """net c (no global average pool, which has a refusal of its own): through the batch-normalisation rule, as for RCN_HIPX_CONV3X3"""
    from mercer_research_amd.convnet import ConvNetError
    net, = twins(P_C, "fp32", 1)
    x, y = batches(net, P_C, 1)[0]
    before = net.plan_of_this_net(P_C[2])
    with pytest.raises(ConvNetError, match=r"-3: .*batch normalisation"):
        net.set_precision("bf16_stored")
    assert net.plan_of_this_net(P_C[2]) == before and "fp32 operands" in before
    step(net, x, y, LR)
    net.close()


@FORMS
def test_cifar_bottleneck_description_trains_at_a_small_batch(pw):
    """bench_convnet.py's cifar_bottleneck at B = 8: create accepts its 29 layers with parameters and the loss falls over a few steps"""
    import torch
    import bench_convnet
    in_shape, layers, _ = bench_convnet.CONFIGS["cifar_bottleneck"]
    assert sum(l[0] not in ("pool", "global_avgpool") for l in layers) == 29
    net = make_net((in_shape, layers, 8), "fp32")
    net.set_option("pw", pw)
    net.init_params(1)
    rng = np.random.default_rng(0)
    x, y = dev(net, rng.standard_normal((8,) + in_shape).astype(np.float32)), dev(net, rng.integers(0, 10, 8).astype(np.int32))
    loss = torch.zeros(1, dtype=torch.float32, device=net.device)
    seen = []
    for _ in range(6):
        step(net, x, y, 0.02, loss)
        seen.append(float(loss.item()))
    assert np.isfinite(seen).all() and seen[-1] < 0.7 * seen[0], seen
    net.close()
