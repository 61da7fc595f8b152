"""The 1x1 convolution without a GPU (include/rcn_hipx.h: RCN_HIPX_CONV1X1 = ("conv1x1_linear", Cout)): every refusal of a description,
what is accepted, the plans of the nets of tests/test_gpu_convnet_pw.py and of bench_convnet.py's cifar_bottleneck by the plan's own text
(the streaming kernel with the input read once and more than once, its looping grid, the implicit-GEMM form with and without split-K,
both precisions, the skip's add directly behind the input gradient of every block's first layer), the state layout, and the float64
torch twin of the GPU tests (tests/_pw_ref.py): pinned on a case worked out by hand, shown to see four mutants, and the conditions the GPU
comparison rests on -- the margin condition of tests/_twin_checks.py's comparison and the bf16 twin agreeing with itself in float32."""
import contextlib
import io
import re

import numpy as np
import pytest
from _convnet_util import convnet_loaded, plan_lines  # noqa: F401  (fixture)
from _pw_ref import (LOOPING, NETS, OPTIONS, P_B, P_D, PW, RTOL, RTOL_2, SEEDS, STEPS, X_SPEC, PwNet, bottleneck, case, compare, exact_case, layout, n_logical, param_shapes,
                     tensor_slices)
from _twin_checks import twin_schedule

KIND = "RCN_HIPX_CONV1X1"
BN = (("bn_relu",),)
REFUSALS = [
    # (input shape, layers, status, layer index named, a word of the message)
    ((4, 4, 3), ((PW, 32),) + BN + (("dense", 4),), -3, 0, "multiple of 32, not 3"),
    ((4, 4, 1), ((PW, 32),) + BN + (("dense", 4),), -3, 0, "multiple of 32, not 1"),
    ((4, 4, 3), (("conv", 48 - 16), ("pool",), (PW, 48)) + BN + (("dense", 4),), -3, 2, "positive multiple of 32"),
    ((4, 4, 32), ((PW, 0),) + BN + (("dense", 4),), -3, 0, "positive multiple of 32"),
    ((4, 4, 32), ((PW, -32),) + BN + (("dense", 4),), -3, 0, "positive multiple of 32"),
    ((4, 4, 32), (("dense_relu", 32), (PW, 32)) + BN + (("dense", 4),), -2, 1, "after a dense layer or a global average pool"),
    ((4, 4, 32), (("conv", 32), ("global_avgpool",), (PW, 32)) + BN + (("dense", 4),), -2, 2, "after a dense layer or a global average pool"),
    ((4, 4, 32), ((PW, 32), ("dense", 4)), -2, 0, "followed directly by a batch-normalisation layer"),
    ((4, 4, 32), ((PW, 32), ("conv", 32), ("dense", 4)), -2, 0, "followed directly by a batch-normalisation layer"),
    ((4, 4, 32), ((PW, 32), (PW, 32)) + BN + (("dense", 4),), -2, 0, "followed directly by a batch-normalisation layer"),
    ((4, 4, 32), ((PW, 32), ("pool",), ("dense", 4)), -2, 0, "followed directly by a batch-normalisation layer"),
    ((4, 4, 32), ((PW, 32), ("global_avgpool",), ("dense", 4)), -2, 0, "followed directly by a batch-normalisation layer"),
    ((4, 4, 32), (("conv", 32), (PW, 32)), -2, 1, "followed directly by a batch-normalisation layer"),
]


@pytest.mark.parametrize("in_shape,layers,status,index,word", REFUSALS, ids=[f"{r[2]}-{r[4].replace(' ', '-').replace(',', '')}-{k}" for k, r in enumerate(REFUSALS)])
def test_refusals_name_the_layer_and_the_reason(convnet, in_shape, layers, status, index, word):
    for fn in (convnet.plan, convnet.plan_eval, lambda *a: convnet.plan(*a, buckets=0)):
        with pytest.raises(convnet.ConvNetError, match=rf": {status}: layer {index} \({KIND}\): .*{word}"):
            fn(in_shape, layers, 2)
    with pytest.raises(convnet.ConvNetError, match=rf"rcn_hipx_state_layout: {status}$"):
        convnet.state_layout(in_shape, layers)


def test_what_stays_refused_and_what_is_accepted(convnet):
    """bf16 storage: through batch normalisation's rule, as for RCN_HIPX_CONV3X3; a 1x1 map is never a skip's source (it is not normalised)"""
    for fn in (convnet.plan, convnet.plan_eval):
        with pytest.raises(convnet.ConvNetError, match=r"-3: .*batch normalisation"):
            fn(*NETS["c"], "bf16_stored")
    with pytest.raises(convnet.ConvNetError, match=r": -2: layer 4 \(RCN_HIPX_BN_ADD_RELU\): .*the skip's source, layer 1, must be"):
        convnet.plan((4, 4, 32), (("conv", 32), (PW, 32), ("bn_relu",), ("conv_linear", 32), ("bn_add_relu", 3), ("dense", 4)), 2)
    # accepted: as layer 0 on a 32-channel input (no input gradient); above a pool (epilogue 0); above a bn_add_relu_down (epilogue 3)
    first = plan_lines(convnet.plan((4, 4, 32), ((PW, 64),) + BN + (("dense", 4),), 2))
    assert [l for l in first if l.startswith("conv1x1")] == [l for l in first if l.startswith("conv1x1") and " epi 1:" in l] and sum(l.startswith("conv1x1") for l in first) == 1
    assert sum(l.startswith("wgrad conv1x1 4x4x32->64") for l in first) == 1
    pool = plan_lines(convnet.plan(*NETS["c"]))
    assert any(l.startswith("conv1x1 4x4x128->32 epi 0:") for l in pool), pool
    down = (("conv", 32), ("conv_linear_s2", 64), ("bn_relu",), ("conv_linear", 64), ("bn_add_relu_down", 4), (PW, 32)) + BN + (("global_avgpool",), ("dense", 4))
    lines = plan_lines(convnet.plan((8, 8, 32), down, 2))
    assert any(l.startswith("conv1x1 4x4x64->32 epi 1:") for l in lines) and any(l.startswith("conv1x1 4x4x32->64 epi 3:") for l in lines), lines
    assert convnet.state_layout((8, 8, 32), down).layers[5].kind == 10


# ---- plan text ------------------------------------------------------------------------------------------------------------------------------

def _pw(lines):
    return [l for l in lines if l.startswith("conv1x1")]


def _plan(convnet, monkeypatch, spec, precision="fp32", **env):
    for k, v in env.items():
        monkeypatch.setenv("RCN_HIPX_" + k.upper(), str(v))
    lines = plan_lines(convnet.plan(spec[0], spec[1], spec[2], precision))
    for k in env:
        monkeypatch.delenv("RCN_HIPX_" + k.upper())
    return lines


@pytest.mark.parametrize("precision", ["fp32", "bf16"])
@pytest.mark.parametrize("name", sorted(NETS))
def test_every_1x1_gemm_has_its_line_in_both_forms(convnet, monkeypatch, name, precision):
    """forward (epi 1) and input gradient (epi 3 or 0; none for layer 0) per 1x1 layer from select_pw's own describe, a weight gradient on
    the KS = 1 kernels; pw = 1: k_pw in the operand precision, pw = 0: the implicit-GEMM form; evaluation: the forward lines alone"""
    spec = NETS[name]
    layers = spec[1]
    n_pw, first = sum(l[0] == PW for l in layers), layers[0][0] == PW
    for pw in (1, 0):
        lines = _plan(convnet, monkeypatch, spec, precision, pw=pw)
        got = _pw(lines)
        assert len(got) == 2 * n_pw - first and sum(" epi 1:" in l for l in got) == n_pw, got
        want = ("k_pw<bf16, " if precision == "bf16" else "k_pw<f32, ") if pw else ("k_conv_fwd_bf16<1, tile, " if precision == "bf16" else "k_conv_fwd<1, tile, ")
        assert all(want in l and "input read" in l for l in got), got
        assert all(("staged once in LDS" in l and "row blocks of 128 rows" in l) == bool(pw) for l in got), got
        wg = [l for l in lines if l.startswith("wgrad conv1x1")]
        assert len(wg) == n_pw and all(("k_conv_wgrad_bf16<1, " if precision == "bf16" else "k_conv_wgrad<1, tile, ") in l for l in wg), wg
        monkeypatch.setenv("RCN_HIPX_PW", str(pw))
        ev = _pw(plan_lines(convnet.plan_eval(spec[0], spec[1], spec[2], precision)))
        monkeypatch.delenv("RCN_HIPX_PW")
        assert len(ev) == n_pw and all(" epi 1:" in l and want in l for l in ev), ev


def test_forms_the_gpu_cases_reach(convnet, monkeypatch):
    """the input read once (nets a, b, c; K x Cout fits the slice) and more than once (net d's 256 -> 256: four slices of 64 in fp32, two of
    128 in bf16, forward and input gradient); a partial row block (a: M = 72), full and partial (b: M = 300 = 3 blocks), fewer rows than a
    block (c: M = 32); the looping grid (d under halo_f32_slots = 3: sixteen row blocks on three workgroups, on one per slice where the
    slices outnumber the slots); pw = 0: split-K on net d's K = 256 layer and none on its K = 32 layer; b's three weight-gradient chunks"""
    for name, blocks in (("a", 1), ("b", 3), ("c", 1), ("d", 16)):
        got = _pw(_plan(convnet, monkeypatch, NETS[name], pw=1))
        assert all(f", {blocks} row blocks of 128 rows on a resident grid" in l for l in got), got
        if name != "d":
            assert all(l.endswith("input read once") for l in got), got
    for precision, nb, passes in (("fp32", 64, 4), ("bf16", 128, 2)):
        got = _pw(_plan(convnet, monkeypatch, P_D, precision, pw=1))
        assert len(got) == 3 and got[0].startswith("conv1x1 16x16x32->256 epi 1:") and "weights [32][256] staged once" in got[0] and got[0].endswith("input read once"), got
        for l, epi in ((got[1], 1), (got[2], 3)):
            assert l.startswith(f"conv1x1 16x16x256->256 epi {epi}:") and f"weights [256][{nb}] staged once" in l and l.endswith(f"input read {passes} times ({passes} column slices)"), l
        loop = _pw(_plan(convnet, monkeypatch, P_D, precision, pw=1, **dict(LOOPING)))
        assert "on 3 looping workgroups per slice" in loop[0] and all(f"on {max(1, 3 // passes)} looping workgroups per slice" in l for l in loop[1:]), loop
    for precision, kernel in (("fp32", "k_conv_fwd<1, tile, 64>"), ("bf16", "k_conv_fwd_bf16<1, tile, 128>")):
        got = _pw(_plan(convnet, monkeypatch, P_D, precision, pw=0))
        assert kernel in got[0] and "split-K" not in got[0], got[0]
        assert all(kernel + " split-K 2 + k_splitk_epilogue" in l for l in got[1:]), got
    assert OPTIONS["b"] == (("pix_per_chunk", 128),)
    wg = [l for l in _plan(convnet, monkeypatch, P_B, pix_per_chunk=128) if l.startswith("wgrad conv1x1")]
    assert len(wg) == 2 and all(l.endswith(", 3 chunks") for l in wg), wg


def _skip_lines_stand_behind_the_input_gradient(lines, sources):
    at = [i for i, l in enumerate(lines) if l.startswith("skip-bwd")]
    assert len(at) == len(sources), (len(at), sources)
    for i, src in zip(at, sources):
        assert f"into layer {src}'s gradient" in lines[i] and f"then gated by layer {src}'s output" in lines[i], lines[i]
        assert lines[i - 1].startswith("conv1x1") and " epi 3:" in lines[i - 1] and lines[i + 1].startswith("wgrad conv1x1"), lines[i - 1:i + 2]


@pytest.mark.parametrize("pw", [1, 0])
def test_the_skip_add_stands_directly_behind_the_first_layers_input_gradient(convnet, monkeypatch, pw):
    """the source of a bottleneck's skip is the layer below the block's first 1x1 layer: that layer's input-gradient launch writes all of
    the source's gradient, the add follows it at once, and the 1x1 layer's weight gradient comes after"""
    for precision in ("fp32", "bf16"):
        _skip_lines_stand_behind_the_input_gradient(_plan(convnet, monkeypatch, P_B, precision, pw=pw), [1])
    # in the bucket plan the add stays in the iteration of the layer above the source
    monkeypatch.setenv("RCN_HIPX_PW", str(pw))
    lines = [l.strip() for l in convnet.plan(P_B[0], P_B[1], P_B[2], buckets=0).splitlines()]
    i, = [k for k, x in enumerate(lines) if x.startswith("skip-bwd")]
    opened = [x for x in lines[:i] if x.startswith("bucket") and "done" not in x][-1]
    assert re.fullmatch(r"bucket \d+: layers 2 \.\. 2", opened), opened


def test_cifar_bottleneck_plans_and_lists_29_reduction_jobs(convnet, monkeypatch):
    import bench_convnet
    in_shape, layers, B = bench_convnet.CONFIGS["cifar_bottleneck"]
    want = (("conv_linear", 128), ("bn_relu",)) + bottleneck(128) + bottleneck(128) + (("pool",), (PW, 256), ("bn_relu",)) + bottleneck(256) + bottleneck(256) + (("pool",), ("global_avgpool",), ("dense", 10))
    assert (in_shape, B) == ((32, 32, 3), 512) and tuple(layers) == want and sum(l[0] not in ("pool", "global_avgpool") for l in layers) == 29
    for precision in ("fp32", "bf16"):
        for pw in (1, 0):
            lines = _plan(convnet, monkeypatch, (in_shape, layers, B), precision, pw=pw)
            assert lines[-1].startswith("update: k_reduce_all,") and " 29 layers' slabs in one launch" in lines[-1], lines[-1]
            assert len(_pw(lines)) == 18 and sum(l.startswith("wgrad conv1x1") for l in lines) == 9
            _skip_lines_stand_behind_the_input_gradient(lines, [22, 16, 7, 1])
    once = [l for l in _pw(_plan(convnet, monkeypatch, (in_shape, layers, B), pw=1)) if l.endswith("input read once")]
    assert len(once) == 16                                  # all but the widening 128 -> 256 and its input gradient 256 -> 128 (two slices each in fp32)
    assert all(l.endswith("input read once") for l in _pw(_plan(convnet, monkeypatch, (in_shape, layers, B), "bf16", pw=1)))
    # the default is the implicit-GEMM form in both precisions (measured)
    assert all("k_conv_fwd<1, tile, " in l for l in _pw(_plan(convnet, monkeypatch, (in_shape, layers, B)))) and all("k_conv_fwd_bf16<1, tile, " in l for l in _pw(_plan(convnet, monkeypatch, (in_shape, layers, B), "bf16")))


# ---- state layout, HBM floor ----------------------------------------------------------------------------------------------------------------

def test_state_layout_stays_version_1_and_carries_the_kind(convnet):
    in_shape, layers, _ = P_B
    d = convnet.state_layout(in_shape, layers)
    assert convnet.KIND[PW] == 10 and d.version == 1
    assert [d.layers[i].kind for i in range(d.n_layers)] == [convnet.KIND[l[0]] for l in layers]
    assert (d.layers[2].kind, d.layers[2].out) == (10, 32) and (d.layers[6].kind, d.layers[6].out) == (10, 128) and (d.layers[7].kind, d.layers[7].out) == (6, 6)
    assert d.shape_and_layers() == (in_shape, [tuple(l) for l in layers])
    sl = tensor_slices(in_shape, layers)
    with_params = [i for i, l in enumerate(layers) if l[0] not in ("pool", "global_avgpool")]
    assert d.n_log == n_logical(in_shape, layers) and [d.layer_off[i] for i in with_params] == [s[0].start for s in sl]
    assert param_shapes(in_shape, layout(layers))[2:7:2] == [(128, 32), (9 * 32, 32), (32, 128)]
    body = np.zeros(int(d.body_bytes), dtype=np.uint8)
    d2, _, extra = convnet.read_state_file(convnet.write_state_file(d, body, b"x"))
    assert d2.shape_and_layers() == (in_shape, [tuple(l) for l in layers]) and extra == b"x"


def test_hbm_floor_counts_a_1x1_layer_as_a_convolution_with_a_cin_by_cout_matrix(convnet):
    floor = convnet.ConvNet.step_hbm_floor_bytes
    mk = lambda in_shape, layers: type("N", (), {"in_shape": in_shape, "layers": [tuple(l) for l in layers]})()
    a = floor(mk((8, 8, 32), (("conv", 32), (PW, 64), ("bn_relu",), ("dense", 4))), 2)
    b = floor(mk((8, 8, 32), (("conv", 32), ("conv_linear", 64), ("bn_relu",), ("dense", 4))), 2)
    assert b - a == 3 * 8 * 32 * 64 * 4                     # the same maps three times; eight taps fewer of the weights, read twice and written once


# ---- the twin, pinned by hand ---------------------------------------------------------------------------------------------------------------

def test_twin_1x1_convolution_on_a_hand_computed_case():
    """Two samples of a 1 x 2 x 32 map, 32 -> 32: z[m] = x[m] W + b per pixel m with W[K = Cin][Cout] as the flat layout holds it; under
    L = sum_m v[m] . z[m]: dx[m] = W v[m], dW = sum_m x[m] (outer) v[m], db = sum_m v[m]."""
    C = Co = 32
    rng = np.random.default_rng(0)
    x = rng.standard_normal((2, 1, 2, C))
    W, b, v = rng.standard_normal((C, Co)) * 0.2, rng.standard_normal(Co), rng.standard_normal((2, 1, 2, Co))
    layers = ((PW, Co), ("bn_relu",), ("dense", 1))
    flat = np.concatenate([W.ravel(), b, np.ones(Co), np.zeros(Co), np.zeros(2 * Co), [0.0]])
    net = PwNet((1, 2, C), layers, flat)
    net.forward(x, False)
    z = net.outs[0]
    assert tuple(z.shape) == (2, Co, 1, 2)
    assert np.allclose(z.detach().numpy().transpose(0, 2, 3, 1), x @ W + b, rtol=0, atol=1e-12)
    assert np.abs(x @ W + b - (x @ W.T + b)).max() > 0.1, "W and its transpose differ on this case"
    for m in net.mods:
        m.zero_grad()
    t = net.torch.from_numpy(np.ascontiguousarray(x.transpose(0, 3, 1, 2))).requires_grad_(True)
    (net._conv(net.mods[0], t) * net.torch.from_numpy(np.ascontiguousarray(v.transpose(0, 3, 1, 2)))).sum().backward()
    assert np.allclose(t.grad.numpy().transpose(0, 2, 3, 1), v @ W.T, rtol=0, atol=1e-12)
    g = net._flat(lambda p: p.grad if p.grad is not None else net.torch.zeros_like(p))
    ws, bs = tensor_slices((1, 2, C), layers)[0]
    assert np.allclose(g[ws].reshape(C, Co), np.einsum("nhwc,nhwd->cd", x, v), rtol=0, atol=1e-12)
    assert np.allclose(g[bs], v.sum((0, 1, 2)), rtol=0, atol=1e-12)


def _share(got, ref, in_shape, layers, rtol):
    """the worst |d| / allowance of close_per_tensor, without asserting"""
    worst = 0.0
    for ws, bs in tensor_slices(in_shape, layers):
        for t in (ws, bs):
            worst = max(worst, float(np.abs(got[t] - ref[t]).max()) / (rtol * max(1e-3, float(np.abs(ref[t]).max())) + 1e-6))
    return worst


# a square bottleneck on the hand case's map: a ReLU convolution below the block's first layer (its gate), the skip from it, 32 -> 32 throughout
HAND = ((1, 2, 32), (("conv", 32), (PW, 32), ("bn_relu",), ("conv_linear", 32), ("bn_relu",), (PW, 32), ("bn_add_relu", 6), ("dense", 3)), 2)
MUTANTS = ["w_transposed", "drop_bias_grad", "open_gate_below", "drop_skip_share"]


@pytest.mark.parametrize("mutant", MUTANTS)
def test_the_twin_sees_each_mutant(mutant):
    """Each mutant moves the twin's gradient by more than an fp32 allowance (2e-4 of a tensor's scale + 1e-6) of _twin_checks.compare on the
    two-sample 1 x 2 x 32 case.  The gradient is taken on the running statistics (mean 0, variance 1): under batch statistics the
    gradient of a bias in front of batch normalisation is zero in exact arithmetic, and no comparison could see it dropped."""
    import torch
    in_shape, layers, B = HAND
    from _pw_ref import random_params
    flat = random_params(np.random.default_rng(0), in_shape, layers)
    rng = np.random.default_rng(1)
    x, y = rng.standard_normal((B,) + in_shape), rng.integers(0, 3, B)

    def grad(**kw):
        net = PwNet(in_shape, layers, flat, **kw)
        for m in net.mods:
            m.zero_grad()
        torch.nn.functional.cross_entropy(net.forward(x, False), torch.from_numpy(y.astype(np.int64))).backward()
        return net._flat(lambda p: p.grad if p.grad is not None else torch.zeros_like(p))
    share = _share(grad(**{mutant: True}), grad(), in_shape, layers, RTOL["fp32"])
    print(f"{mutant}: the gradient moves by {share:.0f} allowances")
    assert share > 1.0, (mutant, share)


# ---- the conditions the GPU comparison rests on, from the twin alone ------------------------------------------------------------------------

@pytest.mark.parametrize("precision", ["fp32", "bf16"])
@pytest.mark.parametrize("name", sorted(NETS))
def test_margin_condition_of_the_comparison_holds(name, precision):
    """_twin_checks.compare asserts margin > 4 * rtol2 * scale before it compares the correct count: at the seeds in use, from the twin alone"""
    in_shape, layers, _ = NETS[name]
    flat, x, y = case(name)
    ref = twin_schedule(PwNet(in_shape, layers, flat, operand="bf16" if precision == "bf16" else "f64"), x, y, STEPS)
    print(f"net {name} {precision} seeds {SEEDS[name]}: margin {ref['margin']:.4f}, scale {ref['scale']:.3f}, bound {4 * RTOL_2[precision] * ref['scale']:.4f}")
    assert ref["margin"] > 4 * RTOL_2[precision] * ref["scale"], (name, precision, ref["margin"], ref["scale"])


@pytest.mark.parametrize("name", sorted(NETS))
def test_bf16_twin_agrees_with_itself_in_float32(name):
    """The reference's own error, as tests/test_convnet_stride_plan.py measures it: the bf16-operand twin evaluated in float32 stays within
    0.3 of every bf16 allowance of the comparison the GPU test makes against the same twin in float64."""
    in_shape, layers, _ = NETS[name]
    flat, x, y = case(name)
    ref = twin_schedule(PwNet(in_shape, layers, flat, operand="bf16"), x, y, STEPS)
    f32 = twin_schedule(PwNet(in_shape, layers, flat, operand="bf16", arithmetic="float32"), x, y, STEPS)
    with contextlib.redirect_stdout(io.StringIO()):
        share = compare(NETS[name], f32, ref, RTOL["bf16"], RTOL_2["bf16"], STEPS, f"net {name} twin in float32")
    print(f"net {name}: the bf16 twin in float32 against itself in float64: worst share of an allowance = {share:.3f}")
    assert share < 0.3, (name, share)


def test_the_exact_net_is_exact_in_every_precision():
    """tests/_pw_ref.py's small-integer net: every operand is an integer of at most 8 bits (exact in bf16), every sum below 2^24 (exact in
    float32 in any order), and the twin's float64 evaluation on the running statistics gives NumPy's integers"""
    flat, stats, x, want, a2 = exact_case()
    assert np.abs(x).max() <= 2 and a2.max() <= 255 and np.abs(want).max() < 2 ** 24
    w = flat[tensor_slices(X_SPEC[0], X_SPEC[1])[0][0]]
    assert set(np.unique(w)) <= {-1.0, 0.0, 1.0}
    net = PwNet(X_SPEC[0], X_SPEC[1], flat)
    net.set_bn_stats(stats)
    z = net.logits(x, train=False)
    # float64 batch normalisation: 1 / sqrt(var + eps) is 1 to 2e-8, so the twin agrees to that and rounds to the integers
    assert np.array_equal(np.rint(z), want) and np.abs(z - want).max() < 1e-3 * max(1.0, np.abs(want).max())
