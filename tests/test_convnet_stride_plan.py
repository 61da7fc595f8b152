"""The two downsampling layer kinds without a GPU (include/rcn_hipx.h: RCN_HIPX_CONV3X3_S2 = ("conv_linear_s2", Cout),
RCN_HIPX_BN_ADD_RELU_DOWN = ("bn_add_relu_down", d)): every refusal of a description, the plans of the nets of
tests/test_gpu_convnet_stride.py (no LDS-tiled kernel, no fused pool and no pooled operand for a strided layer under any tiling; the
parity classes of the input gradient; which kernel forms the GPU cases reach), the state layout, and the float64 torch twin of the GPU
tests (tests/_stride_ref.py): pinned on two cases worked out by hand, shown to see four mutants at the GPU cases' shapes and seeds, and
the margin condition of tests/_twin_checks.py's comparison for every GPU case."""
import re

import numpy as np
import pytest
from _convnet_util import convnet_loaded, plan_lines  # noqa: F401  (fixture)
from _stride_ref import D_A, D_B, D_C, NETS, OPTIONS, RTOL, RTOL_2, STEPS, StrideNet, case, down, layout, resnet14
from _torch_ref import n_logical, tensor_slices
from _twin_checks import twin_schedule

S2, DOWN = "RCN_HIPX_CONV3X3_S2", "RCN_HIPX_BN_ADD_RELU_DOWN"
REFUSALS = [
    # (input shape, layers, status, layer index named, its kind, a word of the message)
    ((5, 4, 32), (("conv_linear_s2", 32), ("bn_relu",), ("dense", 4)), -3, 0, S2, "even height and width"),
    ((4, 6 + 1, 32), (("conv_linear_s2", 32), ("bn_relu",), ("dense", 4)), -3, 0, S2, "even height and width"),
    ((4, 4, 3), (("conv_linear_s2", 32), ("bn_relu",), ("dense", 4)), -3, 0, S2, "multiple of 32"),
    ((4, 4, 32), (("conv", 32), ("conv_linear_s2", 48), ("bn_relu",), ("dense", 4)), -3, 1, S2, "positive multiple of 32"),
    ((4, 4, 32), (("conv_linear_s2", 0), ("bn_relu",), ("dense", 4)), -3, 0, S2, "positive multiple of 32"),
    ((4, 4, 32), (("dense_relu", 32), ("conv_linear_s2", 32), ("bn_relu",), ("dense", 4)), -2, 1, S2, "after a dense layer or a global average pool"),
    ((4, 4, 32), (("conv", 32), ("global_avgpool",), ("conv_linear_s2", 32), ("bn_relu",), ("dense", 4)), -2, 2, S2, "after a dense layer or a global average pool"),
    ((4, 4, 32), (("conv_linear_s2", 32), ("dense", 4)), -2, 0, S2, "followed directly by a batch-normalisation layer"),
    ((4, 4, 32), (("conv_linear_s2", 32), ("conv", 32), ("dense", 4)), -2, 0, S2, "followed directly by a batch-normalisation layer"),
    ((4, 4, 32), (("conv_linear_s2", 32), ("global_avgpool",), ("dense", 4)), -2, 0, S2, "followed directly by a batch-normalisation layer"),
    ((4, 4, 32), (("conv", 32), ("conv_linear_s2", 32)), -2, 1, S2, "followed directly by a batch-normalisation layer"),
    # the shortcut: the source must be exactly twice as high and wide, and no wider than this layer
    ((4, 4, 32), (("conv", 32), ("conv_linear", 32), ("bn_add_relu_down", 2), ("dense", 4)), -2, 2, DOWN, "exactly twice"),
    ((8, 8, 32), (("conv", 32), ("conv_linear_s2", 32), ("bn_relu",), ("conv_linear_s2", 32), ("bn_add_relu_down", 4), ("dense", 4)), -2, 4, DOWN, "exactly twice"),
    ((4, 4, 32), (("conv", 64), ("conv_linear_s2", 32), ("bn_add_relu_down", 2), ("dense", 4)), -2, 2, DOWN, "more channels"),
    # ... and bn_add_relu's own rules hold for it
    ((4, 4, 32), (("conv", 32), ("conv", 32), ("bn_add_relu_down", 2), ("dense", 4)), -2, 2, DOWN, "directly follow"),
    ((4, 4, 32), (("conv", 32), ("conv_linear_s2", 32), ("bn_add_relu_down", 1), ("dense", 4)), -1, 2, DOWN, "at least 2"),
    ((4, 4, 32), (("conv", 32), ("conv_linear_s2", 32), ("bn_add_relu_down", 3), ("dense", 4)), -2, 2, DOWN, "net's input"),
    ((4, 4, 32), (("conv", 32), ("pool",), ("conv_linear", 32), ("bn_add_relu_down", 3), ("dense", 4)), -2, 3, DOWN, "max-pool behind it"),
]


@pytest.mark.parametrize("in_shape,layers,status,index,kind,word", REFUSALS, ids=[f"{r[2]}-{r[5].replace(' ', '-')}-{k}" for k, r in enumerate(REFUSALS)])
def test_refusals_name_the_layer_and_the_reason(convnet, in_shape, layers, status, index, kind, word):
    for fn in (convnet.plan, convnet.plan_eval):
        with pytest.raises(convnet.ConvNetError, match=rf": {status}: layer {index} \({kind}\): .*{word}"):
            fn(in_shape, layers, 2)
    with pytest.raises(convnet.ConvNetError, match=rf"rcn_hipx_state_layout: {status}$"):
        convnet.state_layout(in_shape, layers)


def test_what_stays_refused(convnet):
    """an identity skip across a resolution change keeps its own refusal; bf16 storage keeps batch normalisation's"""
    with pytest.raises(convnet.ConvNetError, match=r": -2: layer 4 \(RCN_HIPX_BN_ADD_RELU\): .*output shape"):
        convnet.plan((4, 4, 32), (("conv", 32), ("conv_linear_s2", 32), ("bn_relu",), ("conv_linear", 32), ("bn_add_relu", 4), ("dense", 4)), 2)
    for fn in (convnet.plan, convnet.plan_eval):
        with pytest.raises(convnet.ConvNetError, match=r"-3: .*batch normalisation"):
            fn(*D_C, "bf16_stored")
    # (C - Cs) % 8 != 0 cannot be described: both widths are multiples of 32 (the rule guards the 16-byte window for a later narrower kind)
    assert all(l[1] % 32 == 0 for s in NETS.values() for l in s[1] if l[0] in ("conv", "conv_linear", "conv_linear_s2"))


# ---- plan text ------------------------------------------------------------------------------------------------------------------------------

def _strided(lines):
    """the lines of a plan that belong to strided layers' three GEMMs"""
    return [l for l in lines if l.startswith(("conv3x3/2", "dgrad conv3x3/2", "wgrad conv3x3/2"))]


@pytest.mark.parametrize("halo", [0, 1])
@pytest.mark.parametrize("tiling", ["gemm", "auto", "lds"])
@pytest.mark.parametrize("precision", ["fp32", "bf16"])
@pytest.mark.parametrize("name", sorted(NETS))
def test_a_strided_layer_never_shows_an_lds_tiled_kernel(convnet, monkeypatch, name, precision, tiling, halo):
    monkeypatch.setenv("RCN_HIPX_HALO", str(halo))
    in_shape, layers, B = NETS[name]
    lines = plan_lines(convnet.plan(in_shape, layers, B, precision, tiling))
    n_s2 = sum(l[0] == "conv_linear_s2" for l in layers)
    first = layers[0][0] == "conv_linear_s2"
    st = _strided(lines)
    assert len(st) == 3 * n_s2 - first, st                 # forward, input gradient (not for layer 0), weight gradient
    for l in st:
        assert "halo" not in l and "k_conv1" not in l and "pooled" not in l and " epi 4" not in l and "items" not in l, l
        assert ("ConvShapeS2T>" if l.startswith("dgrad") else "ConvShapeS2>") in l, l
    assert sum(l.startswith("conv3x3/2") and " epi 1:" in l for l in st) == n_s2
    ev = [l for l in plan_lines(convnet.plan_eval(in_shape, layers, B, precision, tiling)) if "conv3x3/2" in l]
    assert len(ev) == n_s2 and all(l.startswith("conv3x3/2") and "ConvShapeS2>" in l for l in ev), ev


@pytest.mark.parametrize("name", ["a", "b", "c"])
def test_the_input_gradient_line_shows_four_classes(convnet, name):
    in_shape, layers, B = NETS[name]
    for precision in ("fp32", "bf16"):
        for l in [x for x in plan_lines(convnet.plan(in_shape, layers, B, precision)) if x.startswith("dgrad conv3x3/2")]:
            oh, ow, H, W = map(int, re.match(r"dgrad conv3x3/2 (\d+)x(\d+)x\d+->(\d+)x(\d+)x", l).groups())
            assert (H, W) == (2 * oh, 2 * ow) and "one launch" in l
            tiles = [int(t) for t in re.findall(r"taps?: (\d+) tiles", l)]
            taps = [int(t) for t in re.findall(r"\) (\d) taps?:", l)]
            rows = B * H * W // 4                           # M_in / 4 rows per class
            assert taps == [4, 2, 2, 1] and tiles == [-(-rows // 128)] * 4 and sum(tiles) == 4 * -(-rows // 128), l


def test_split_k_applies_to_the_strided_forward_where_tiles_are_few(convnet):
    """kept: the strided forward is the stride-1 body on M_out rows.  Nets a, b, c have 1 - 3 output tiles: split-K; net d has 256: none"""
    for name, want in (("a", True), ("b", True), ("c", True), ("d", False)):
        in_shape, layers, B = NETS[name]
        fw = [l for l in plan_lines(convnet.plan(in_shape, layers, B)) if l.startswith("conv3x3/2")]
        assert fw and all(("split-K" in l and "k_splitk_epilogue" in l) == want and ("no split-K" in l) != want for l in fw), fw
    assert any("256 output tiles, no split-K" in l for l in plan_lines(convnet.plan(*NETS["d"])))


def test_the_shortcut_lines(convnet):
    """forward: the apply launch names its source, the subsample and the channel window; backward: the strided add directly behind the
    parity launch of layer S + 1, in front of that layer's weight gradient, with the identity skip's gate words"""
    in_shape, layers, B = D_B
    lines = plan_lines(convnet.plan(in_shape, layers, B))
    adds = [l for l in lines if l.startswith("bn-add-relu") and "_down" in l]
    assert len(adds) == 2 and "skip: the output of layer 5, subsampled (2h, 2w), its 32 channels at 16 .. 47)" in adds[0] and "its 64 channels at 32 .. 95)" in adds[1], adds
    at = [i for i, l in enumerate(lines) if l.startswith("skip-bwd") and "k_skip_bwd_add_down" in l]
    assert len(at) == 2
    for i, src in zip(at, (9, 5)):
        assert f"into layer {src}'s gradient" in lines[i] and f"then gated by layer {src}'s output" in lines[i], lines[i]
        assert lines[i - 1].startswith("dgrad conv3x3/2") and " epi 3:" in lines[i - 1] and lines[i + 1].startswith("wgrad conv3x3/2"), lines[i - 1:i + 2]
    # a pool source is not gated: epilogue 0 and the ungated add
    lines = plan_lines(convnet.plan(*D_C))
    i, = [k for k, l in enumerate(lines) if l.startswith("skip-bwd")]
    assert "ungated: layer 1 is a pool" in lines[i] and "gated here (out > 0)" in lines[i] and " epi 0:" in lines[i - 1], lines[i - 1:i + 1]
    ev = [l for l in plan_lines(convnet.plan_eval(*D_B)) if "_down<eval>" in l]
    assert len(ev) == 2 and all("subsampled (2h, 2w)" in l for l in ev)


def test_bucket_plan_keeps_the_strided_add_in_the_iteration_of_the_layer_above_the_source(convnet):
    in_shape, layers, B = D_B
    lines = [l.strip() for l in convnet.plan(in_shape, layers, B, buckets=0).splitlines()]
    for s in (9, 5):
        i, = [k for k, x in enumerate(lines) if x.startswith("skip-bwd") and f"into layer {s}'s gradient" in x]
        opened = [x for x in lines[:i] if x.startswith("bucket") and "done" not in x][-1]
        assert re.fullmatch(rf"bucket \d+: layers {s + 1} \.\. {s + 1}", opened), opened


def test_resnet14_plans_and_lists_27_reduction_jobs(convnet):
    in_shape, layers, B = resnet14()
    assert sum(l[0] not in ("pool", "global_avgpool") for l in layers) == 27
    for precision in ("fp32", "bf16"):
        lines = plan_lines(convnet.plan(in_shape, layers, B, precision))
        assert lines[-1].startswith("update: k_reduce_all,") and " 27 layers' slabs in one launch" in lines[-1], lines[-1]
        assert len(_strided(lines)) == 6 and sum(l.startswith("skip-bwd") for l in lines) == 6
    import bench_convnet
    assert bench_convnet.CONFIGS["cifar_resnet14"] == (in_shape, layers, B)


# ---- forms reached --------------------------------------------------------------------------------------------------------------------------

def test_every_strided_kernel_form_is_reached_by_a_gpu_case(convnet, monkeypatch):
    """What the selectors (csrc/convnet_select.hpp: select_conv_s2, select_dgrad_s2, select_wgrad_s2) can return for a strided layer, read
    off their code: forward fp32 column blocks 64 / 32, bf16 128 / 64 / 32, with and without split-K; input gradient 64 / 32 in either
    precision, epilogues 3 and 0; weight gradient 64 / 32 in either precision (bf16 always three waves).  The plans of the GPU cases of
    tests/test_gpu_convnet_stride.py reach each."""
    from test_gpu_convnet_stride import CASES
    seen = set()
    for name, precision, options in CASES:
        for k, v in options:
            monkeypatch.setenv("RCN_HIPX_" + k.upper(), str(v))
        in_shape, layers, B = NETS[name]
        for l in _strided(plan_lines(convnet.plan(in_shape, layers, B, precision))):
            kernel, args = re.search(r": (k_\w+)<([^>]*)>", l).groups()
            args = [a.strip() for a in args.split(",")]
            bn = int(args[2] if kernel in ("k_conv_fwd", "k_conv_fwd_bf16", "k_conv_wgrad") else args[1])
            seen.add((l.split()[0], kernel, bn))
            if l.startswith("conv3x3/2"):
                seen.add(("split-K", "no split-K" not in l))
            if l.startswith("dgrad"):
                seen.add(("dgrad epi", int(re.search(r" epi (\d):", l).group(1))))
        for k, _ in options:
            monkeypatch.delenv("RCN_HIPX_" + k.upper())
    want = {("conv3x3/2", "k_conv_fwd", 64), ("conv3x3/2", "k_conv_fwd", 32), ("conv3x3/2", "k_conv_fwd_bf16", 128), ("conv3x3/2", "k_conv_fwd_bf16", 64),
            ("conv3x3/2", "k_conv_fwd_bf16", 32), ("split-K", True), ("split-K", False),
            ("dgrad", "k_conv_fwd", 64), ("dgrad", "k_conv_fwd", 32), ("dgrad", "k_conv_fwd_bf16", 64), ("dgrad", "k_conv_fwd_bf16", 32), ("dgrad epi", 3), ("dgrad epi", 0),
            ("wgrad", "k_conv_wgrad", 64), ("wgrad", "k_conv_wgrad", 32), ("wgrad", "k_conv_wgrad_bf16", 64), ("wgrad", "k_conv_wgrad_bf16", 32)}
    assert seen == want, (sorted(map(str, want - seen)), sorted(map(str, seen - want)))
    # net b's option: three weight-gradient chunks of 128 output pixels on the 12x20 -> 6x10 layer (M_out = 300), the last partial
    monkeypatch.setenv("RCN_HIPX_PIX_PER_CHUNK", "128")
    assert any(l.startswith("wgrad conv3x3/2 12x20x32->6x10x64") and l.endswith(", 3 chunks") for l in plan_lines(convnet.plan(*D_B)))
    assert OPTIONS["b"] == (("pix_per_chunk", 128),)


# ---- state layout ---------------------------------------------------------------------------------------------------------------------------

def test_state_layout_stays_version_1_and_carries_both_kinds(convnet):
    in_shape, layers, _ = D_B
    d = convnet.state_layout(in_shape, layers)
    assert convnet.KIND["conv_linear_s2"] == 8 and convnet.KIND["bn_add_relu_down"] == 9 and d.version == 1
    assert [d.layers[i].kind for i in range(d.n_layers)] == [convnet.KIND[l[0]] for l in layers]
    assert (d.layers[6].kind, d.layers[6].out) == (8, 64) and (d.layers[9].kind, d.layers[9].out) == (9, 4) and (d.layers[13].kind, d.layers[13].out) == (9, 4)
    assert d.shape_and_layers() == (in_shape, [tuple(l) for l in layers])
    assert d.n_log == n_logical(in_shape, layout(layers)) and d.layer_off[6] == tensor_slices(in_shape, layout(layers))[6][0].start
    body = np.zeros(int(d.body_bytes), dtype=np.uint8)
    d2, _, extra = convnet.read_state_file(convnet.write_state_file(d, body, b"x"))
    assert d2.shape_and_layers() == (in_shape, [tuple(l) for l in layers]) and extra == b"x"


def test_hbm_floor_counts_a_quarter_map_for_the_strided_layer_and_the_shortcut(convnet):
    floor = convnet.ConvNet.step_hbm_floor_bytes
    mk = lambda in_shape, layers: type("N", (), {"in_shape": in_shape, "layers": [tuple(l) for l in layers]})()
    a = floor(mk((8, 8, 32), (("conv", 32), ("conv_linear_s2", 64), ("bn_relu",), ("dense", 4))), 2)
    b = floor(mk((8, 8, 32), (("conv", 32), ("conv_linear", 64), ("bn_relu",), ("pool",), ("dense", 4))), 2)
    # stride 1 + pool writes and reads the full 8x8x64 map; the strided layer only its 4x4x64 one
    assert a < b
    with_skip = floor(mk((8, 8, 32), (("conv", 32),) + down(64) + (("dense", 4),)), 2)
    without = floor(mk((8, 8, 32), (("conv", 32), ("conv_linear_s2", 64), ("bn_relu",), ("conv_linear", 64), ("bn_relu",), ("dense", 4))), 2)
    assert with_skip - without == 2 * 4 * (4 * 4 * 32 * 4)     # four passes over the source's 32 channels at 4 x 4 pixels


# ---- the twin, pinned by hand ---------------------------------------------------------------------------------------------------------------

def test_twin_strided_convolution_on_a_hand_computed_case():
    """One sample, a 2 x 2 x C map: the stride-2 output is ONE pixel, centred on input (0, 0), and only the four taps kh, kw in {1, 2} are
    in range: z[co] = b[co] + sum over those taps of x[kh - 1][kw - 1] . W[kh][kw][:, co].  Its gradients under L = v . z: dx[ih][iw] =
    W[ih + 1][iw + 1] v, dW[kh][kw] = x[kh - 1][kw - 1] (outer) v for the four live taps and zero for the five others."""
    C, Co = 32, 32
    rng = np.random.default_rng(0)
    x = rng.standard_normal((1, 2, 2, C))
    W, b, v = rng.standard_normal((3, 3, C, Co)) * 0.1, rng.standard_normal(Co), rng.standard_normal(Co)
    layers = (("conv_linear_s2", Co), ("bn_relu",), ("dense", 1))
    flat = np.concatenate([W.ravel(), b, np.ones(Co), np.zeros(Co), np.zeros(Co), [0.0]])
    net = StrideNet((2, 2, C), layers, flat)
    net.forward(x, False)
    z = net.outs[0]
    assert tuple(z.shape) == (1, Co, 1, 1)
    want = b + sum(x[0, kh - 1, kw - 1] @ W[kh, kw] for kh in (1, 2) for kw in (1, 2))
    assert np.allclose(z.detach().numpy().ravel(), want, rtol=0, atol=1e-12)
    for m in net.mods:
        m.zero_grad()
    t = net.torch.from_numpy(np.ascontiguousarray(x.transpose(0, 3, 1, 2))).requires_grad_(True)
    (net.mods[0](t)[0, :, 0, 0] * net.torch.from_numpy(v)).sum().backward()
    dx = t.grad.numpy().transpose(0, 2, 3, 1)[0]
    for ih in range(2):
        for iw in range(2):
            assert np.allclose(dx[ih, iw], W[ih + 1, iw + 1] @ v, rtol=0, atol=1e-12), (ih, iw)
    dW = net.mods[0].weight.grad.numpy().transpose(2, 3, 1, 0)      # [kh][kw][ci][co]
    for kh in range(3):
        for kw in range(3):
            live = kh >= 1 and kw >= 1
            assert np.allclose(dW[kh, kw], np.outer(x[0, kh - 1, kw - 1], v) if live else 0.0, rtol=0, atol=1e-12), (kh, kw)
    # the mutant reads rows 2 oh + kh: centred on (1, 1), taps kh, kw in {0, 1} live
    other = StrideNet((2, 2, C), layers, flat, pad_other_side=True)
    other.forward(x, False)
    want_other = b + sum(x[0, kh, kw] @ W[kh, kw] for kh in (0, 1) for kw in (0, 1))
    assert np.allclose(other.outs[0].detach().numpy().ravel(), want_other, rtol=0, atol=1e-12) and np.abs(want_other - want).max() > 0.1


def test_twin_shortcut_on_a_hand_computed_case():
    """2 x 2 -> 1 x 1 with Cs = 32 < C = 64, the main path shut (the strided convolution's weights are zero, so no gradient reaches the
    source through it) and evaluation statistics: y = relu(k + s'), k the block's constant, s'[c] = s[0][0][c - 16] inside 16 .. 47; under
    L = w . y the source's gradient is w[16 + c'] where y > 0 at pixel (0, 0), and exactly zero at the three other pixels."""
    C, Cs = 64, 32
    rng = np.random.default_rng(1)
    eye = np.zeros((9 * Cs, Cs)); eye[4 * Cs:5 * Cs] = np.eye(Cs)
    g2, b2 = 0.5 + rng.random(C), rng.standard_normal(C) * 0.5
    w = rng.standard_normal(C)
    layers = (("conv", Cs),) + down(C) + (("dense", 1),)
    flat = np.concatenate([eye.ravel(), np.zeros(Cs), np.zeros(9 * Cs * C), np.zeros(C), np.ones(C), np.zeros(C),
                           np.zeros(9 * C * C), np.zeros(C), g2, b2, w, [0.0]])
    x = 0.5 + rng.random((2, 2, 2, Cs))                       # positive: the source s = relu(x) = x
    net = StrideNet((2, 2, Cs), layers, flat)
    z = net.forward(x, False)
    net.outs[0].retain_grad()
    z.sum().backward()
    k = b2                                                     # bn2(conv2(relu(bn1(0)))) with zero weights and biases: beta
    sp = np.zeros((2, C)); sp[:, 16:48] = x[:, 0, 0, :]
    y = np.maximum(0.0, k + sp)
    assert np.allclose(net.outs[4].detach().numpy().reshape(2, C), y, rtol=0, atol=1e-12)
    got = net.outs[0].grad.numpy().transpose(0, 2, 3, 1)       # [b][h][w][c']
    want = ((y > 0) * w)[:, 16:48]
    assert np.allclose(got[:, 0, 0], want, rtol=0, atol=1e-12), np.abs(got[:, 0, 0] - want).max()
    assert (want == 0).any() and (np.abs(want) > 0.01).sum() > 32, "the window holds both closed and open ReLUs"
    assert not got[:, 0, 1].any() and not got[:, 1, 0].any() and not got[:, 1, 1].any()
    assert (y[:, :16] == np.maximum(0.0, k[:16])).all() and (y[:, 48:] == np.maximum(0.0, k[48:])).all()
    # the mutants: sampled at (1, 1), or the window at 0 .. 31
    odd = StrideNet((2, 2, Cs), layers, flat, sample_odd=True)
    odd.forward(x, False)
    spo = np.zeros((2, C)); spo[:, 16:48] = x[:, 1, 1, :]
    assert np.allclose(odd.outs[4].detach().numpy().reshape(2, C), np.maximum(0.0, k + spo), rtol=0, atol=1e-12)
    lo0 = StrideNet((2, 2, Cs), layers, flat, lo_zero=True)
    lo0.forward(x, False)
    sp0 = np.zeros((2, C)); sp0[:, :32] = x[:, 0, 0, :]
    assert np.allclose(lo0.outs[4].detach().numpy().reshape(2, C), np.maximum(0.0, k + sp0), rtol=0, atol=1e-12)


# ---- the reference sees the mutants; the margin ---------------------------------------------------------------------------------------------

def _share(got, ref, in_shape, layers, rtol):
    """the worst |d| / allowance of _torch_ref.close_per_tensor, without asserting"""
    worst = 0.0
    for ws, bs in tensor_slices(in_shape, layout(layers)):
        for t in (ws, bs):
            worst = max(worst, float(np.abs(got[t] - ref[t]).max()) / (rtol * max(1e-3, float(np.abs(ref[t]).max())) + 1e-6))
    return worst


@pytest.fixture(scope="module")
def true_grads():
    """the float64 twin's gradient of every GPU case's net, once"""
    out = {}
    for name, (in_shape, layers, _) in NETS.items():
        flat, x, y = case(name)
        out[name] = StrideNet(in_shape, layers, flat).loss_and_grads(x, y)[2]
    return out


# (mutant, the nets it applies to): the padding side wherever a strided layer has a layer below or above to show it; the shortcut's mutants
# where there is one (lo = 0 only where Cs < C); the source gate where the source has one (net c's source is a pool)
MUTANTS = [("pad_other_side", "abcd"), ("sample_odd", "abc"), ("lo_zero", "ab"), ("gate_source", "ab")]


@pytest.mark.parametrize("mutant,nets", MUTANTS, ids=[m for m, _ in MUTANTS])
def test_the_twin_sees_each_mutant(true_grads, mutant, nets):
    """At the GPU cases' shapes and seeds each mutant moves the twin's gradient by more than 100 allowances of close_per_tensor at the fp32
    bound (2e-4): a device that computed the mutant could not pass the comparison."""
    for name in nets:
        in_shape, layers, _ = NETS[name]
        flat, x, y = case(name)
        g = StrideNet(in_shape, layers, flat, **{mutant: mutant != "gate_source"}).loss_and_grads(x, y)[2]
        share = _share(g, true_grads[name], in_shape, layers, RTOL["fp32"])
        print(f"net {name}, {mutant}: the gradient moves by {share:.0f} allowances")
        assert share > 100.0, (name, mutant, share)


def test_net_d_has_no_relu_tie_within_float32_reach():
    """The device decides the bn_relu layer's gate on a float32 pre-activation whose error is a few 1e-7 (a 288-term fp32 contraction, then
    four roundings of the apply pass at |values| <= 16); the twin decides it in float64.  No element of net d's map is closer to zero than 1e-6."""
    import torch
    in_shape, layers, _ = NETS["d"]
    flat, x, _ = case("d")
    net = StrideNet(in_shape, layers, flat)
    with torch.no_grad():
        net.forward(x, True)
        pre = net.mods[1](net.outs[0]).numpy()
    print(f"net d: smallest |pre-activation| = {np.abs(pre).min():.3e} of {pre.size}, largest {np.abs(pre).max():.2f}")
    assert pre.size == 128 * 16 * 16 * 64 and np.abs(pre).min() > 1e-6 and np.abs(pre).max() < 16


def _self_share(name, seeds=None):
    """The bf16-operand twin of net `name` run through the schedule in float32 arithmetic against itself in float64, by
    _twin_checks.compare at the bf16 bounds: (worst share of an allowance, None), or (None, the first quantity that misses)"""
    import contextlib
    import io
    from _stride_ref import layout_spec
    from _twin_checks import compare
    in_shape, layers, _ = NETS[name]
    flat, x, y = case(name, seeds)
    ref = twin_schedule(StrideNet(in_shape, layers, flat, operand="bf16"), x, y, STEPS)
    f32 = twin_schedule(StrideNet(in_shape, layers, flat, operand="bf16", arithmetic="float32"), x, y, STEPS)
    if not ref["margin"] > 4 * RTOL_2["bf16"] * ref["scale"]:
        return None, ("margin", ref["margin"], ref["scale"])
    try:
        with contextlib.redirect_stdout(io.StringIO()):
            return compare(layout_spec(NETS[name]), f32, ref, RTOL["bf16"], RTOL_2["bf16"], STEPS, f"net {name} twin in float32"), None
    except AssertionError as e:
        return None, e.args[0]


@pytest.mark.parametrize("name", ["a", "b", "c"])
def test_bf16_twin_agrees_with_itself_in_float32(name):
    """The reference's own error: the float64 twin with bf16-rounded operands models a device that computes in float32, and an activation
    whose float32 and float64 values straddle a bf16 rounding boundary enters the next GEMM 2^-8 of itself apart.  At the seeds in use the
    twin evaluated in float32 stays within 0.3 of every bf16 allowance of the comparison the GPU test makes."""
    share, miss = _self_share(name)
    print(f"net {name}: the bf16 twin in float32 against itself in float64: worst share of an allowance = {share}, miss = {miss}")
    assert miss is None and share < 0.3, (name, share, miss)


def test_net_b_at_its_first_seeds_misses_its_own_float64_self():
    """Seeds (3, 4), the first tried for net b: in ONE training pass the twin's two arithmetics are further apart than the bf16 allowance
    in some gradient tensor, and their training logits about as far as the device measured against the float64 twin there
    (profiles/trackx_stride_tests.txt: 7.46 allowances on the first layer's weight gradient, training logits 3.66e-3 apart).  That run
    measured the reference; so would a comparison at most other seeds (the margin condition also fails at these)."""
    in_shape, layers, _ = NETS["b"]
    flat, x, y = case("b", (3, 4))
    _, z64, g64 = StrideNet(in_shape, layers, flat, operand="bf16").loss_and_grads(x, y)
    _, z32, g32 = StrideNet(in_shape, layers, flat, operand="bf16", arithmetic="float32").loss_and_grads(x, y)
    d, share = float(np.abs(z32 - z64).max()), _share(g32, g64, in_shape, layers, RTOL["bf16"])
    print(f"net b at seeds (3, 4), float32 against float64 arithmetic: training logits |d| = {d:.3e}, gradient worst share of a bf16 allowance = {share:.2f}")
    assert 1e-3 < d < 1e-2 and share > 1.0, (d, share)
    # ... and at the seeds in use the same figure is small
    flat, x, y = case("b")
    _, _, g64 = StrideNet(in_shape, layers, flat, operand="bf16").loss_and_grads(x, y)
    _, _, g32 = StrideNet(in_shape, layers, flat, operand="bf16", arithmetic="float32").loss_and_grads(x, y)
    assert _share(g32, g64, in_shape, layers, RTOL["bf16"]) < 0.3


@pytest.mark.parametrize("precision", ["fp32", "bf16"])
@pytest.mark.parametrize("name", sorted(NETS))
def test_margin_condition_of_the_comparison_holds(name, precision):
    """_twin_checks.compare asserts margin > 4 * rtol2 * scale before it compares the correct count: from the twin alone"""
    in_shape, layers, _ = NETS[name]
    flat, x, y = case(name)
    ref = twin_schedule(StrideNet(in_shape, layers, flat, operand="bf16" if precision == "bf16" else "f64"), x, y, STEPS)
    print(f"net {name} {precision}: margin {ref['margin']:.4f}, scale {ref['scale']:.3f}, bound {4 * RTOL_2[precision] * ref['scale']:.4f}")
    assert ref["margin"] > 4 * RTOL_2[precision] * ref["scale"], (name, precision, ref["margin"], ref["scale"])
