"""The depthwise 3x3 convolution without a GPU (include/rcn_hipx.h: RCN_HIPX_DWCONV3X3 = ("dwconv_linear",)): every refusal of a description
by status and message from the plan, the evaluation plan, the bucket plan and the state layout; what is accepted; the plans of the nets of
tests/test_gpu_convnet_dw.py and of bench_convnet.py's cifar_sep by the plan's own text (the stencil kernel's tiles and its looping grid,
the skip's add directly behind the gated input gradient and in front of the weight gradient, fp32 arithmetic in bf16 mode with no operand
copies, the weight gradient's chunks); from those lines, that each GPU case reaches what its comment names; the state layout and the HBM
floor; and the float64 torch twin of the GPU tests (tests/_dw_ref.py): pinned on a case worked out by hand, shown to see six mutants, and
the conditions the GPU comparison rests on -- the margin condition of tests/_twin_checks.py's comparison and the bf16 twin agreeing with
itself in float32."""
import contextlib
import io
import re

import numpy as np
import pytest
from _convnet_util import convnet_loaded, plan_lines  # noqa: F401  (fixture)
from _dw_ref import (DW, LOOPING, NETS, OPTIONS, PW, RTOL, RTOL_2, SEEDS, STEPS, W_B, W_C, W_D, W_S, X_SPEC, DwNet, case, compare, exact_case, layout, n_logical, param_shapes, random_params,
                     residual, separable, tensor_slices)
from _twin_checks import twin_schedule

KIND = "RCN_HIPX_DWCONV3X3"
BN = (("bn_relu",),)
REFUSALS = [
    # (input shape, layers, status, layer index named, a word of the message)
    ((4, 4, 3), ((DW,),) + BN + (("dense", 4),), -3, 0, "multiple of 32, not 3"),
    ((4, 4, 1), ((DW,),) + BN + (("dense", 4),), -3, 0, "multiple of 32, not 1"),
    ((4, 4, 3), (("conv", 32), ("pool",), ("conv", 64), (PW, 32), ("bn_relu",), ("conv", 32), (DW, 48)) + BN + (("dense", 4),), -2, 6, "32.* not 48"),
    ((4, 4, 32), ((DW, 64),) + BN + (("dense", 4),), -2, 0, "out must be 0 or the input channels 32 .*, not 64"),
    ((4, 4, 32), ((DW, -32),) + BN + (("dense", 4),), -2, 0, "out must be 0 or the input channels 32 .*, not -32"),
    ((4, 4, 32), (("dense_relu", 32), (DW,)) + BN + (("dense", 4),), -2, 1, "after a dense layer or a global average pool"),
    ((4, 4, 32), (("conv", 32), ("global_avgpool",), (DW,)) + BN + (("dense", 4),), -2, 2, "after a dense layer or a global average pool"),
    ((4, 4, 32), ((DW,), ("dense", 4)), -2, 0, "followed directly by a batch-normalisation layer"),
    ((4, 4, 32), ((DW,), ("conv", 32), ("dense", 4)), -2, 0, "followed directly by a batch-normalisation layer"),
    ((4, 4, 32), ((DW,), (DW,)) + BN + (("dense", 4),), -2, 0, "followed directly by a batch-normalisation layer"),
    ((4, 4, 32), ((DW,), (PW, 32)) + BN + (("dense", 4),), -2, 0, "followed directly by a batch-normalisation layer"),
    ((4, 4, 32), ((DW,), ("pool",), ("dense", 4)), -2, 0, "followed directly by a batch-normalisation layer"),
    ((4, 4, 32), ((DW,), ("global_avgpool",), ("dense", 4)), -2, 0, "followed directly by a batch-normalisation layer"),
    ((4, 4, 32), (("conv", 32), (DW,)), -2, 1, "followed directly by a batch-normalisation layer"),
]


@pytest.mark.parametrize("in_shape,layers,status,index,word", REFUSALS, ids=[f"{r[2]}-{re.sub('[^a-z0-9]+', '-', r[4])}-{k}" for k, r in enumerate(REFUSALS)])
def test_refusals_name_the_layer_and_the_reason(convnet, in_shape, layers, status, index, word):
    for fn in (convnet.plan, convnet.plan_eval, lambda *a: convnet.plan(*a, buckets=0)):
        with pytest.raises(convnet.ConvNetError, match=rf": {status}: layer {index} \({KIND}\): .*{word}"):
            fn(in_shape, layers, 2)
    with pytest.raises(convnet.ConvNetError, match=rf"rcn_hipx_state_layout: {status}$"):
        convnet.state_layout(in_shape, layers)


def test_what_stays_refused_and_what_is_accepted(convnet):
    """bf16 storage: through batch normalisation's rule, as for RCN_HIPX_CONV3X3; a depthwise map is never a skip's source (it is not
    normalised): refused by the source rule as it stands"""
    for fn in (convnet.plan, convnet.plan_eval):
        with pytest.raises(convnet.ConvNetError, match=r"-3: .*batch normalisation"):
            fn(*W_S, "bf16_stored")
    with pytest.raises(convnet.ConvNetError, match=r": -2: layer 4 \(RCN_HIPX_BN_ADD_RELU\): .*the skip's source, layer 1, must be"):
        convnet.plan((4, 4, 32), (("conv", 32), (DW,), ("bn_relu",), ("conv_linear", 32), ("bn_add_relu", 3), ("dense", 4)), 2)
    # accepted: as layer 0 on a 32-channel input (no input gradient), out = 0 and out = Cin alike
    for first_layer in ((DW,), (DW, 0), (DW, 32)):
        first = plan_lines(convnet.plan((4, 4, 32), (first_layer,) + BN + (("dense", 4),), 2))
        dw = [l for l in first if l.startswith("dwconv")]
        assert len(dw) == 1 and dw[0].startswith("dwconv 3x3 4x4x32 epi 1: k_dw<1>"), first
        assert sum(l.startswith("wgrad dwconv 3x3 4x4x32:") for l in first) == 1
        assert convnet.state_layout((4, 4, 32), (first_layer,) + BN + (("dense", 4),)).layers[0].out == 32
    # above a pool (epilogue 0), above a ReLU convolution and above batch normalisation of either skip kind (epilogue 3)
    pool = plan_lines(convnet.plan(*W_C))
    assert any(l.startswith("dwconv 3x3 2x2x32 epi 0: k_dw<0>") for l in pool), pool
    add = (("conv", 32), ("conv_linear", 32), ("bn_relu",), ("conv_linear", 32), ("bn_add_relu", 4), (DW,)) + BN + (("global_avgpool",), ("dense", 4))
    lines = plan_lines(convnet.plan((8, 8, 32), add, 2))
    assert any(l.startswith("dwconv 3x3 8x8x32 epi 3: k_dw<3>") for l in lines), lines
    down = (("conv", 32), ("conv_linear_s2", 64), ("bn_relu",), ("conv_linear", 64), ("bn_add_relu_down", 4), (DW,)) + BN + (("global_avgpool",), ("dense", 4))
    lines = plan_lines(convnet.plan((8, 8, 32), down, 2))
    assert any(l.startswith("dwconv 3x3 4x4x64 epi 1:") for l in lines) and any(l.startswith("dwconv 3x3 4x4x64 epi 3: k_dw<3>") for l in lines), lines
    assert convnet.state_layout((8, 8, 32), down).layers[5].kind == 11
    # in front of either skip kind: the residual separable block is net b; a depthwise layer directly in front of a bn_add_relu
    direct = (("conv", 32), (DW,), ("bn_relu",), (DW,), ("bn_add_relu", 4), ("global_avgpool",), ("dense", 4))
    assert sum(l.startswith("dwconv") for l in plan_lines(convnet.plan((8, 8, 32), direct, 2))) == 4


# ---- plan text ------------------------------------------------------------------------------------------------------------------------------

def _dw(lines):
    return [l for l in lines if l.startswith("dwconv")]


def _wg(lines):
    return [l for l in lines if l.startswith("wgrad dwconv")]


def _plan(convnet, monkeypatch, spec, precision="fp32", **env):
    for k, v in env.items():
        monkeypatch.setenv("RCN_HIPX_" + k.upper(), str(v))
    lines = plan_lines(convnet.plan(spec[0], spec[1], spec[2], precision))
    for k in env:
        monkeypatch.delenv("RCN_HIPX_" + k.upper())
    return lines


TILES = re.compile(r"tiles of (\d+) rows x 256 pieces of 16 bytes \((\d+) bands x (\d+) slabs per image, (\d+) tiles\), workgroups (.*)$")
CHUNKS = re.compile(r"(\d+) channel groups x (\d+) chunks of (\d+) pixels$")


@pytest.mark.parametrize("precision", ["fp32", "bf16"])
@pytest.mark.parametrize("name", sorted(NETS))
def test_every_depthwise_layer_has_its_lines_and_computes_in_fp32(convnet, monkeypatch, name, precision):
    """forward (epi 1), input gradient (epi 3 or 0; none for layer 0) and weight gradient per depthwise layer from select_dw's own describe,
    the same lines in both precision modes (fp32 arithmetic by kind); evaluation: the forward lines alone; the micro and epoch plans and
    the bucket plan carry them too"""
    spec = NETS[name]
    layers = spec[1]
    n_dw, first = sum(l[0] == DW for l in layers), layers[0][0] == DW
    lines = _plan(convnet, monkeypatch, spec, precision)
    got = _dw(lines)
    assert len(got) == 2 * n_dw - first and sum(" epi 1: k_dw<1>" in l for l in got) == n_dw, got
    assert all("(fp32 arithmetic)" in l and TILES.search(l) for l in got), got
    wg = _wg(lines)
    assert len(wg) == n_dw and all("k_dw_wgrad (fp32 arithmetic)" in l and CHUNKS.search(l) for l in wg), wg
    assert got + wg == _dw(_plan(convnet, monkeypatch, spec, "fp32")) + _wg(_plan(convnet, monkeypatch, spec, "fp32")), "the kind's lines depend on the precision mode"
    ev = _dw(plan_lines(convnet.plan_eval(spec[0], spec[1], spec[2], precision)))
    assert len(ev) == n_dw and all(" epi 1: k_dw<1>" in l for l in ev), ev
    bucket = [l.strip() for l in convnet.plan(spec[0], spec[1], spec[2], precision, buckets=0).splitlines()]
    assert _dw(bucket) == got and _wg(bucket) == wg, bucket


def test_bf16_mode_makes_no_operand_copies_of_a_depthwise_layer(convnet):
    """One k_prep_all_bf16 launch takes 32 jobs, two per GEMM layer behind layer 0.  A net of 16 such layers and a depthwise layer still
    prepares its copies in that one launch: the kind makes none and is not counted; with a 17th GEMM layer it goes to per-launch copies,
    and the count it names is the GEMM layers'"""
    def layers(dense):
        return (("conv", 32), (DW,), ("bn_relu",)) + (("dense_relu", 32),) * (dense - 1) + (("dense", 4),)
    lines = plan_lines(convnet.plan((4, 4, 3), layers(16), 2, "bf16"))
    assert lines[0].startswith("bf16 operand copies of every layer's weights, both orientations: k_prep_all_bf16 (one launch)"), lines[0]
    assert len(_dw(lines)) == 2 and all("(fp32 arithmetic)" in l for l in _dw(lines))
    lines = plan_lines(convnet.plan((4, 4, 3), layers(17), 2, "bf16"))
    assert lines[0].startswith("bf16 operand copies: none prepared (17 matrix layers behind layer 0, one launch takes 16)"), lines[0]


def test_forms_the_gpu_cases_reach(convnet, monkeypatch):
    """From the plan lines, what each GPU case's comment names.
    a: one tile per image, a band taller than the map (H = 3 of 8 rows), epilogue 3.  b: 24 quads per pixel (256 % 24 != 0: a lane's quad
    changes with the tile -- here one slab of 240 pieces, 16 lanes idle), three weight-gradient chunks of 128 pixels over M = 300 (the last
    of 44) x three channel groups, the skip's add behind the gated input gradient.  c: a 2 x 2 map, epilogue 0.  d: layer 0 without an input
    gradient; at C = 256 the forward pass and the gated input gradient in 2 bands (10 = 8 + 2 rows) x 5 slabs (1152 = 4 x 256 + 128 pieces):
    more than one tile in both tiled directions and a multiple of the tile in neither; the weight gradient in twelve chunks of 128 pixels
    over M = 1440 (the last of 32) x eight channel groups -- its channel direction is tiled by 32 and C % 32 == 0 is the layer's own
    condition, so only the pixel direction can be partial; under halo_f32_slots = 3 three workgroups loop over the 80 tiles."""
    def tiles(line):
        th, bands, slabs, items, grid = TILES.search(line).groups()
        return int(th), int(bands), int(slabs), int(items), grid
    a = _dw(_plan(convnet, monkeypatch, NETS["a"]))
    assert [l[:24] for l in a] == ["dwconv 3x3 3x5x32 epi 1:", "dwconv 3x3 3x5x32 epi 3:"] and all(tiles(l)[:4] == (8, 1, 1, 3) for l in a), a
    assert OPTIONS["b"] == (("pix_per_chunk", 128),)
    b = _plan(convnet, monkeypatch, W_B, pix_per_chunk=128)
    assert [l[:25] for l in _dw(b)] == ["dwconv 3x3 6x10x96 epi 1:", "dwconv 3x3 6x10x96 epi 3:"] and all(tiles(l)[:4] == (8, 1, 1, 5) for l in _dw(b)), _dw(b)
    assert 256 % (96 // 4) != 0 and 10 * 96 // 4 == 240
    assert [CHUNKS.search(l).groups() for l in _wg(b)] == [("3", "3", "128")] and W_B[2] * 6 * 10 == 300 == 2 * 128 + 44, _wg(b)
    c = _dw(_plan(convnet, monkeypatch, W_C))
    assert [l[:24] for l in c] == ["dwconv 3x3 2x2x32 epi 1:", "dwconv 3x3 2x2x32 epi 0:"], c
    for env in ({}, dict(LOOPING)):
        lines = _plan(convnet, monkeypatch, W_D, **env)
        d = _dw(lines)
        assert [l[:27] for l in d] == ["dwconv 3x3 10x18x32 epi 1: ", "dwconv 3x3 10x18x256 epi 1:", "dwconv 3x3 10x18x256 epi 3:"], d
        assert tiles(d[0])[:4] == (8, 2, 1, 16) and all(tiles(l)[:4] == (8, 2, 5, 80) for l in d[1:]), d
        assert 10 % 8 != 0 and 10 > 8 and (18 * 256 // 4) % 256 != 0 and 18 * 256 // 4 > 256
        want = "3 looping over the tiles" if env else "a resident grid looping over the tiles"
        assert all(tiles(l)[4] == want for l in d), d
        assert [CHUNKS.search(l).groups() for l in _wg(lines)] == [("8", "12", "128"), ("1", "12", "128")] and W_D[2] * 10 * 18 == 1440 == 11 * 128 + 32, _wg(lines)


def _skip_lines_stand_behind_the_input_gradient(lines, sources):
    at = [i for i, l in enumerate(lines) if l.startswith("skip-bwd")]
    assert len(at) == len(sources), (len(at), sources)
    for i, (src, gated) in zip(at, sources):
        assert f"into layer {src}'s gradient" in lines[i] and (f"then gated by layer {src}'s output" if gated else f"ungated: layer {src} is a pool") in lines[i], lines[i]
        assert lines[i - 1].startswith("dwconv") and (" epi 3:" if gated else " epi 0:") in lines[i - 1] and lines[i + 1].startswith("wgrad dwconv"), lines[i - 1:i + 2]


def test_the_skip_add_stands_directly_behind_the_depthwise_input_gradient(convnet, monkeypatch):
    """the source of a residual separable block's skip is the layer below its depthwise layer: k_dw writes all of the source's gradient,
    every element once, the add follows it at once, and the depthwise weight gradient comes after -- in the bucket plan too, where the add
    stays in the iteration of the layer above the source"""
    for precision in ("fp32", "bf16"):
        _skip_lines_stand_behind_the_input_gradient(_plan(convnet, monkeypatch, W_B, precision), [(1, True)])
    lines = [l.strip() for l in convnet.plan(W_B[0], W_B[1], W_B[2], buckets=0).splitlines()]
    i, = [k for k, x in enumerate(lines) if x.startswith("skip-bwd")]
    assert lines[i - 1].startswith("dwconv 3x3 6x10x96 epi 3:") and lines[i + 1].startswith("wgrad dwconv"), lines[i - 1:i + 2]
    opened = [x for x in lines[:i] if x.startswith("bucket") and "done" not in x][-1]
    assert re.fullmatch(r"bucket \d+: layers 2 \.\. 2", opened), opened


def test_cifar_sep_plans_and_lists_27_reduction_jobs(convnet, monkeypatch):
    import bench_convnet
    in_shape, layers, B = bench_convnet.CONFIGS["cifar_sep"]
    want = (("conv_linear", 64), ("bn_relu",)) + residual(64) + separable(128) + (("pool",),) + residual(128) + separable(256) + (("pool",),) + residual(256) + residual(256) + (("global_avgpool",), ("dense", 10))
    assert (in_shape, B) == ((32, 32, 3), 512) and tuple(layers) == want and sum(l[0] not in ("pool", "global_avgpool") for l in layers) == 27
    for precision in ("fp32", "bf16"):
        lines = _plan(convnet, monkeypatch, (in_shape, layers, B), precision)
        assert lines[-1].startswith("update: k_reduce_all,") and " 27 layers' slabs in one launch" in lines[-1], lines[-1]
        assert len(_dw(lines)) == 12 and len(_wg(lines)) == 6 and all("(fp32 arithmetic)" in l for l in _dw(lines) + _wg(lines))
        # the sources: layer 1 (bn_relu), the two pools (ungated: they gate in their own backward) and the block in front of the last
        _skip_lines_stand_behind_the_input_gradient(lines, [(23, True), (19, False), (10, False), (1, True)])
    # whole-height bands at the benchmark's batch (1024 tiles each: the chip's 256 CUs x 4 workgroups), so no halo row is read twice
    shapes = {(32, 32, 64): 32, (16, 16, 128): 16, (8, 8, 256): 8}
    for l in _dw(_plan(convnet, monkeypatch, (in_shape, layers, B))):
        h, w, c = map(int, re.match(r"dwconv 3x3 (\d+)x(\d+)x(\d+) ", l).groups())
        th, bands, slabs, items, _ = TILES.search(l).groups()
        assert (int(th), int(bands), int(slabs), int(items)) == (shapes[(h, w, c)], 1, 2, 1024), l
    # the epoch plan and the micro plan of a created net are GPU matters; the description's epoch plan is the step's launches behind a gather
    net_free = convnet.plan(in_shape, layers, B, buckets=0)
    assert net_free.count("dwconv 3x3") == 18


# ---- state layout, HBM floor ----------------------------------------------------------------------------------------------------------------

def test_state_layout_stays_version_1_and_carries_the_kind(convnet):
    in_shape, layers, _ = W_B
    d = convnet.state_layout(in_shape, layers)
    assert convnet.KIND[DW] == 11 and d.version == 1
    assert [d.layers[i].kind for i in range(d.n_layers)] == [convnet.KIND[l[0]] for l in layers]
    assert (d.layers[2].kind, d.layers[2].out) == (11, 96) and (d.layers[4].kind, d.layers[4].out) == (10, 96) and (d.layers[5].kind, d.layers[5].out) == (6, 4)
    # the descriptor stores the resolved width: the description it gives back names it, and names the same net
    resolved = [tuple(l) if l[0] != DW else (DW, 96) for l in layers]
    assert d.shape_and_layers() == (in_shape, resolved)
    d_resolved = convnet.state_layout(in_shape, resolved)
    assert [(d_resolved.layers[i].kind, d_resolved.layers[i].out) for i in range(d.n_layers)] == [(d.layers[i].kind, d.layers[i].out) for i in range(d.n_layers)]
    sl = tensor_slices(in_shape, layers)
    with_params = [i for i, l in enumerate(layers) if l[0] not in ("pool", "global_avgpool")]
    assert d.n_log == n_logical(in_shape, layers) and [d.layer_off[i] for i in with_params] == [s[0].start for s in sl]
    assert param_shapes(in_shape, layout(layers))[2:5:2] == [(9, 96), (96, 96)]
    body = np.zeros(int(d.body_bytes), dtype=np.uint8)
    d2, _, extra = convnet.read_state_file(convnet.write_state_file(d, body, b"x"))
    assert d2.shape_and_layers() == (in_shape, resolved) and extra == b"x"


def test_hbm_floor_counts_a_depthwise_layer_as_a_convolution_on_the_same_maps_with_10_c_parameters(convnet):
    floor = convnet.ConvNet.step_hbm_floor_bytes
    mk = lambda in_shape, layers: type("N", (), {"in_shape": in_shape, "layers": [tuple(l) for l in layers]})()
    a = floor(mk((8, 8, 32), (("conv", 32), (DW,), ("bn_relu",), ("dense", 4))), 2)
    b = floor(mk((8, 8, 32), (("conv", 32), ("conv_linear", 32), ("bn_relu",), ("dense", 4))), 2)
    assert b - a == 3 * (9 * 32 * 32 + 32 - 10 * 32) * 4     # the same maps three times; the parameters read twice and written once


# ---- the twin, pinned by hand ---------------------------------------------------------------------------------------------------------------

def _hand(x, W, b):
    """y[n][h][w][c] = b[c] + sum over kh, kw of W[3 kh + kw][c] x[n][h + kh - 1][w + kw - 1][c], zero outside the map: plain loops"""
    N, H, Wd, C = x.shape
    y = np.zeros_like(x)
    for n in range(N):
        for h in range(H):
            for w in range(Wd):
                acc = b.copy()
                for kh in range(3):
                    for kw in range(3):
                        hh, ww = h + kh - 1, w + kw - 1
                        if 0 <= hh < H and 0 <= ww < Wd:
                            acc += W[3 * kh + kw] * x[n, hh, ww]
                y[n, h, w] = acc
    return y


def test_twin_depthwise_convolution_on_a_hand_computed_case():
    """Two samples of a 2 x 3 x 32 map.  Under L = sum v . z: dx[n][h][w] = sum over taps of W[3 kh + kw] v[n][h - kh + 1][w - kw + 1] (the
    taps reversed), dW[t] = sum over pixels of x[pixel + tap t] v[pixel], db = sum v -- all by plain loops"""
    C = 32
    rng = np.random.default_rng(0)
    x, v = rng.standard_normal((2, 2, 3, C)), rng.standard_normal((2, 2, 3, C))
    W, b = rng.standard_normal((9, C)) * 0.3, rng.standard_normal(C)
    layers = ((DW,), ("bn_relu",), ("dense", 1))
    flat = np.concatenate([W.ravel(), b, np.ones(C), np.zeros(C), np.zeros(2 * 3 * C), [0.0]])
    net = DwNet((2, 3, C), layers, flat)
    net.forward(x, False)
    z = net.outs[0]
    assert tuple(z.shape) == (2, C, 2, 3)
    assert np.allclose(z.detach().numpy().transpose(0, 2, 3, 1), _hand(x, W, b), rtol=0, atol=1e-12)
    Wt = W.reshape(3, 3, C).transpose(1, 0, 2).reshape(9, C)
    assert np.abs(_hand(x, W, b) - _hand(x, Wt, b)).max() > 0.1, "the taps and their transpose differ on this case"
    for m in net.mods:
        m.zero_grad()
    t = net.torch.from_numpy(np.ascontiguousarray(x.transpose(0, 3, 1, 2))).requires_grad_(True)
    (net._conv(net.mods[0], t) * net.torch.from_numpy(np.ascontiguousarray(v.transpose(0, 3, 1, 2)))).sum().backward()
    assert np.allclose(t.grad.numpy().transpose(0, 2, 3, 1), _hand(v, W[::-1].copy(), np.zeros(C)), rtol=0, atol=1e-12)      # the same stencil over v with the taps reversed
    assert np.abs(_hand(v, W[::-1].copy(), np.zeros(C)) - _hand(v, W, np.zeros(C))).max() > 0.1, "the taps and their reverse differ on this case"
    g = net._flat(lambda p: p.grad if p.grad is not None else net.torch.zeros_like(p))
    ws, bs = tensor_slices((2, 3, C), layers)[0]
    dW = np.zeros((9, C))
    for kh in range(3):
        for kw in range(3):
            for h in range(2):
                for w in range(3):
                    if 0 <= h + kh - 1 < 2 and 0 <= w + kw - 1 < 3:
                        dW[3 * kh + kw] += (x[:, h + kh - 1, w + kw - 1] * v[:, h, w]).sum(0)
    assert np.allclose(g[ws].reshape(9, C), dW, rtol=0, atol=1e-12)
    assert np.allclose(g[bs], v.sum((0, 1, 2)), rtol=0, atol=1e-12)
    # the bf16 twin does not round this layer's operands
    r = DwNet((2, 3, C), layers, flat, operand="bf16")
    r.forward(x, False)
    assert np.array_equal(r.outs[0].detach().numpy(), z.detach().numpy())


def _share(got, ref, in_shape, layers, rtol):
    """the worst |d| / allowance of close_per_tensor, without asserting"""
    worst = 0.0
    for ws, bs in tensor_slices(in_shape, layers):
        for t in (ws, bs):
            worst = max(worst, float(np.abs(got[t] - ref[t]).max()) / (rtol * max(1e-3, float(np.abs(ref[t]).max())) + 1e-6))
    return worst


# a residual separable block on a 2 x 3 map: a ReLU convolution below the depthwise layer (its gate), the skip from it
HAND = ((2, 3, 32), (("conv", 32), (DW,), ("bn_relu",), (PW, 32), ("bn_add_relu", 4), ("dense", 3)), 2)
MUTANTS = ["taps_transposed", "taps_unreversed", "wrap_border", "drop_bias_grad", "open_gate_below", "drop_skip_share"]


@pytest.mark.parametrize("mutant", MUTANTS)
def test_the_twin_sees_each_mutant(mutant):
    """Each mutant moves the twin's gradient by more than an fp32 allowance (2e-4 of a tensor's scale + 1e-6) of _twin_checks.compare on a
    two-sample 2 x 3 x 32 case at the seeds in use.  The gradient is taken on the running statistics (mean 0, variance 1), as the 1x1 file
    takes it: under batch statistics the gradient of a bias in front of batch normalisation is zero in exact arithmetic, and no comparison
    could see it dropped."""
    import torch
    in_shape, layers, B = HAND
    flat = random_params(np.random.default_rng(0), in_shape, layers)
    rng = np.random.default_rng(1)
    x, y = rng.standard_normal((B,) + in_shape), rng.integers(0, 3, B)

    def grad(**kw):
        net = DwNet(in_shape, layers, flat, **kw)
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
    ref = twin_schedule(DwNet(in_shape, layers, flat, operand="bf16" if precision == "bf16" else "f64"), x, y, STEPS)
    print(f"net {name} {precision} seeds {SEEDS[name]}: margin {ref['margin']:.4f}, scale {ref['scale']:.3f}, bound {4 * RTOL_2[precision] * ref['scale']:.4f}")
    assert ref["margin"] > 4 * RTOL_2[precision] * ref["scale"], (name, precision, ref["margin"], ref["scale"])


@pytest.mark.parametrize("name", sorted(NETS))
def test_bf16_twin_agrees_with_itself_in_float32(name):
    """The reference's own error, as tests/test_convnet_pw_plan.py measures it: the bf16-operand twin evaluated in float32 stays within
    0.3 of every bf16 allowance of the comparison the GPU test makes against the same twin in float64."""
    in_shape, layers, _ = NETS[name]
    flat, x, y = case(name)
    ref = twin_schedule(DwNet(in_shape, layers, flat, operand="bf16"), x, y, STEPS)
    f32 = twin_schedule(DwNet(in_shape, layers, flat, operand="bf16", arithmetic="float32"), x, y, STEPS)
    with contextlib.redirect_stdout(io.StringIO()):
        share = compare(NETS[name], f32, ref, RTOL["bf16"], RTOL_2["bf16"], STEPS, f"net {name} twin in float32")
    print(f"net {name}: the bf16 twin in float32 against itself in float64: worst share of an allowance = {share:.3f}")
    assert share < 0.3, (name, share)


def test_the_exact_net_is_exact_in_every_precision():
    """tests/_dw_ref.py's small-integer net: every operand is an integer of at most 8 bits (exact in bf16), every sum below 2^24 (exact in
    float32 in any order), and the twin's float64 evaluation on the running statistics gives NumPy's integers"""
    flat, stats, x, want, a2 = exact_case()
    assert np.abs(x).max() <= 2 and a2.max() <= 255 and np.abs(want).max() < 2 ** 24
    for ws, _ in tensor_slices(X_SPEC[0], X_SPEC[1])[0:3:2]:
        assert set(np.unique(flat[ws])) <= {-1.0, 0.0, 1.0}
    net = DwNet(X_SPEC[0], X_SPEC[1], flat)
    net.set_bn_stats(stats)
    z = net.logits(x, train=False)
    # float64 batch normalisation: 1 / sqrt(var + eps) is 1 to 2e-8, so the twin agrees to that and rounds to the integers
    assert np.array_equal(np.rint(z), want) and np.abs(z - want).max() < 1e-3 * max(1.0, np.abs(want).max())
