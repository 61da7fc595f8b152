"""The strided depthwise convolution and the two batch-normalisation kinds without a ReLU, without a GPU (include/rcn_hipx.h:
RCN_HIPX_DWCONV3X3_S2 = ("dwconv_linear_s2",), RCN_HIPX_BN = ("bn",), RCN_HIPX_BN_ADD = ("bn_add", d)): every refusal of a description by
status and message from the plan, the evaluation plan, the bucket plan and the state layout; what is accepted; from the plan text of the
nets of tests/test_gpu_convnet_mb.py and of bench_convnet.py's cifar_mbv2 the gating table of the linear kinds (the convolution above a
linear batch normalisation runs epilogue 0, its backward lines say it is ungated, the skip's add stands directly behind the input gradient
of the layer above the source and names the right gate pair for each of the four source kinds) and the tile, band, slab, chunk and looping
form each GPU case names; the HBM floor by hand on two nets, the state layout (rcn_hipx_step_flops takes a created net, so its count by
hand on two nets stands in the GPU file, not here); and the float64 torch twin of the GPU tests
(tests/_mb_ref.py): pinned by plain Python loops on a two-sample 4 x 6 x 32 case, shown to see seven mutants, and the conditions the GPU
comparison rests on -- the margin condition of tests/_twin_checks.py's comparison and the bf16 twin agreeing with itself in float32."""
import contextlib
import io
import re

import numpy as np
import pytest
from _convnet_util import convnet_loaded, plan_lines  # noqa: F401  (fixture)
from _mb_ref import (BN, BNA, DW, DWS2, LOOPING, M_S, NETS, OPTIONS, PW, RTOL, RTOL_2, SEEDS, STEPS, X_SPEC, MbNet, case, compare, exact_case, inverted, inverted_s2, layout, n_logical,
                     param_shapes, random_params, tensor_slices)
from _twin_checks import twin_schedule

S2_KIND, BN_KIND, BNA_KIND = "RCN_HIPX_DWCONV3X3_S2", "RCN_HIPX_BN", "RCN_HIPX_BN_ADD"
BR = (("bn_relu",),)
HEAD = (("global_avgpool",), ("dense", 4))
STEM = (("conv_linear", 32), ("bn_relu",))
REFUSALS = [
    # (input shape, layers, status, layer index named, its kind, a word of the message)
    ((4, 4, 3), ((DWS2,),) + BR + (("dense", 4),), -3, 0, S2_KIND, "multiple of 32, not 3"),
    ((4, 4, 48), ((DWS2,),) + BR + (("dense", 4),), -3, 0, S2_KIND, "multiple of 32, not 48"),
    ((4, 4, 32), ((DWS2, 64),) + BR + (("dense", 4),), -2, 0, S2_KIND, "out must be 0 or the input channels 32 .*, not 64"),
    ((5, 4, 32), ((DWS2,),) + BR + (("dense", 4),), -3, 0, S2_KIND, "a strided convolution needs even height and width, not 5x4"),
    ((4, 6, 3), (("conv", 32), ("pool",), (DWS2,)) + BR + (("dense", 4),), -3, 2, S2_KIND, "a strided convolution needs even height and width, not 2x3"),
    ((4, 4, 32), (("dense_relu", 32), (DWS2,)) + BR + (("dense", 4),), -2, 1, S2_KIND, "after a dense layer or a global average pool"),
    ((4, 4, 32), (("conv", 32), ("global_avgpool",), (DWS2,)) + BR + (("dense", 4),), -2, 2, S2_KIND, "after a dense layer or a global average pool"),
    ((4, 4, 32), ((DWS2,), ("dense", 4)), -2, 0, S2_KIND, r"followed directly by a batch-normalisation layer \(.*RCN_HIPX_BN or RCN_HIPX_BN_ADD\)"),
    ((4, 4, 32), ((DWS2,), ("conv", 32), ("dense", 4)), -2, 0, S2_KIND, "followed directly by a batch-normalisation layer"),
    ((4, 4, 32), ((DWS2,), (PW, 32)) + BR + (("dense", 4),), -2, 0, S2_KIND, "followed directly by a batch-normalisation layer"),
    ((4, 4, 32), ((DWS2,), ("pool",), ("dense", 4)), -2, 0, S2_KIND, "followed directly by a batch-normalisation layer"),
    ((4, 4, 32), (("conv", 32), (DWS2,)), -2, 1, S2_KIND, "followed directly by a batch-normalisation layer"),
    # bn / bn_add: what they follow
    ((4, 4, 3), (("conv", 32), (BN,), ("conv", 32), ("dense", 4)), -2, 1, BN_KIND, "must directly follow a bias-only convolution"),
    ((4, 4, 3), STEM + ((BN,), ("conv", 32), ("dense", 4)), -2, 2, BN_KIND, "must directly follow a bias-only convolution"),
    ((4, 4, 3), (("conv", 32), ("conv", 32), ("conv", 32), (BNA, 2), ("conv", 32), ("dense", 4)), -2, 3, BNA_KIND, "must directly follow a bias-only convolution"),
    # bn_add: the identity-skip rules of bn_add_relu
    ((4, 4, 3), STEM + ((PW, 32), (BNA, 1), ("conv", 32)) + HEAD, -1, 3, BNA_KIND, "at least 2, not 1"),
    ((4, 4, 32), ((PW, 32), (BNA, 2), ("conv", 32)) + HEAD, -2, 1, BNA_KIND, "in front of layer 0"),
    ((4, 4, 3), STEM + ((PW, 64), (BNA, 2), ("conv", 32)) + HEAD, -2, 3, BNA_KIND, "the skip's source, layer 1, has another output shape"),
    ((4, 4, 3), (("conv", 32), ("pool",), (PW, 32), (BNA, 3), ("conv", 32)) + HEAD, -2, 3, BNA_KIND, "the skip's source, layer 0, has a max-pool behind it"),
    ((4, 4, 3), STEM + ((PW, 32), ("bn_relu",), (PW, 32), (BNA, 3), ("conv", 32)) + HEAD, -2, 5, BNA_KIND,
     r"the skip's source, layer 2, must be a RCN_HIPX_CONV3X3_RELU or RCN_HIPX_MAXPOOL2 layer or a batch-normalisation layer of any kind \(.*RCN_HIPX_BN or RCN_HIPX_BN_ADD\)"),
    ((4, 4, 3), STEM + ((PW, 32), (BNA, 2), (PW, 32), (BNA, 4), ("conv", 32)) + HEAD, -3, 5, BNA_KIND, "already feeds the skip of layer 3"),
    # a linear batch normalisation's consumer: a convolution, nothing else; the message names the linear layer
    ((4, 4, 3), STEM + ((PW, 32), (BN,), ("pool",), ("dense", 4)), -2, 3, BN_KIND, "without a ReLU must be followed directly by a convolution of any kind, not by a RCN_HIPX_MAXPOOL2"),
    ((4, 4, 3), STEM + ((PW, 32), (BN,)) + HEAD, -2, 3, BN_KIND, "without a ReLU must be followed directly by a convolution of any kind, not by a RCN_HIPX_GLOBAL_AVGPOOL"),
    ((4, 4, 3), STEM + ((PW, 32), (BN,), ("dense_relu", 32), ("dense", 4)), -2, 3, BN_KIND, "without a ReLU must be followed directly by a convolution of any kind, not by a RCN_HIPX_DENSE_RELU"),
    ((4, 4, 3), STEM + ((PW, 32), (BN,), ("dense", 4)), -2, 3, BN_KIND, "without a ReLU must be followed directly by a convolution of any kind, not by a RCN_HIPX_DENSE "),
    ((4, 4, 3), STEM + ((PW, 32), (BNA, 2), ("pool",), ("dense", 4)), -2, 3, BNA_KIND, "without a ReLU must be followed directly by a convolution of any kind, not by a RCN_HIPX_MAXPOOL2"),
    ((4, 4, 3), STEM + ((PW, 32), (BNA, 2)) + HEAD, -2, 3, BNA_KIND, "without a ReLU must be followed directly by a convolution of any kind, not by a RCN_HIPX_GLOBAL_AVGPOOL"),
    ((4, 4, 3), STEM + ((PW, 32), (BN,)), -2, 3, BN_KIND, "without a ReLU must be followed directly by a convolution of any kind, and the last layer must be"),
    ((4, 4, 3), STEM + ((PW, 32), (BNA, 2)), -2, 3, BNA_KIND, "without a ReLU must be followed directly by a convolution of any kind, and the last layer must be"),
]


@pytest.mark.parametrize("in_shape,layers,status,index,kind,word", REFUSALS, ids=[f"{r[2]}-{r[4][9:].lower()}-{k}" for k, r in enumerate(REFUSALS)])
def test_refusals_name_the_layer_and_the_reason(convnet, in_shape, layers, status, index, kind, word):
    for fn in (convnet.plan, convnet.plan_eval, lambda *a: convnet.plan(*a, buckets=0)):
        with pytest.raises(convnet.ConvNetError, match=rf": {status}: layer {index} \({kind}\): .*{word}"):
            fn(in_shape, layers, 2)
    with pytest.raises(convnet.ConvNetError, match=rf"rcn_hipx_state_layout: {status}$"):
        convnet.state_layout(in_shape, layers)


def test_the_older_kinds_keep_their_sentences(convnet):
    """the sentences that list kinds stand as they stood: the new kinds are named only in the new kinds' own messages"""
    with pytest.raises(convnet.ConvNetError) as e:
        convnet.plan((4, 4, 32), ((DW,), ("conv", 32), ("dense", 4)), 2)
    assert str(e.value).endswith("it must be followed directly by a batch-normalisation layer (RCN_HIPX_BN_RELU, RCN_HIPX_BN_ADD_RELU or RCN_HIPX_BN_ADD_RELU_DOWN)"), str(e.value)
    with pytest.raises(convnet.ConvNetError) as e:
        convnet.plan((4, 4, 3), STEM + ((PW, 32), ("bn_relu",), (PW, 32), ("bn_add_relu", 3)) + HEAD, 2)
    assert str(e.value).endswith("must be a RCN_HIPX_CONV3X3_RELU, RCN_HIPX_BN_RELU, RCN_HIPX_BN_ADD_RELU or RCN_HIPX_MAXPOOL2 layer (a RCN_HIPX_CONV3X3 map is not yet normalised)"), str(e.value)
    for fn in (convnet.plan, convnet.plan_eval):
        with pytest.raises(convnet.ConvNetError, match=r"-3: .*batch normalisation"):
            fn(*M_S, "bf16_stored")


def _s2(lines):
    return [l for l in lines if l.startswith("dwconv 3x3/2") or l.startswith("dgrad dwconv 3x3/2")]


def _wg(lines):
    return [l for l in lines if l.startswith("wgrad dwconv 3x3/2")]


def test_what_is_accepted(convnet):
    # the strided layer as layer 0 on 32 channels (no input gradient), out = 0 and out = Cin alike; the descriptor stores the resolved width
    for first_layer in ((DWS2,), (DWS2, 0), (DWS2, 32)):
        lines = plan_lines(convnet.plan((4, 4, 32), (first_layer,) + BR + (("dense", 4),), 2))
        assert [l.split(" (fp32")[0] for l in _s2(lines)] == ["dwconv 3x3/2 4x4x32->2x2x32 epi 1: k_dw_s2_fwd"] and len(_wg(lines)) == 1, lines
        d = convnet.state_layout((4, 4, 32), (first_layer,) + BR + (("dense", 4),))
        assert (d.layers[0].kind, d.layers[0].out) == (14, 32) and d.shape_and_layers()[1][0] == (DWS2, 32)
    # above a pool (epilogue 0) and above each of the five batch-normalisation kinds (3 behind a ReLU, 0 behind none)
    assert any(l.startswith("dgrad dwconv 3x3/2 1x1x32->2x2x32 epi 0:") for l in plan_lines(convnet.plan(*NETS["b"])))
    tail = ((DWS2,),) + BR + HEAD
    above = {"bn_relu": (STEM, 3), "bn_add_relu": (STEM + ((PW, 32), ("bn_add_relu", 2)), 3),
             "bn_add_relu_down": ((("conv", 32), ("conv_linear_s2", 32), ("bn_add_relu_down", 2)), 3),
             BN: (STEM + ((PW, 32), (BN,)), 0), BNA: (STEM + ((PW, 32), (BNA, 2)), 0)}
    for kind, (front, epi) in above.items():
        lines = plan_lines(convnet.plan((8, 8, 3), front + tail, 2))
        assert sum(l.startswith("dgrad dwconv 3x3/2 ") and f" epi {epi}: k_dw_s2_dgrad<{epi}>" in l for l in lines) == 1, (kind, lines)
    # in front of bn_relu (net a), of bn, and of bn_add_relu_down (the option-A shortcut of the layer in front of it); an identity skip
    # cannot end a strided layer's block: its source would have the unhalved shape
    assert convnet.plan((8, 8, 3), (("conv", 32), (DWS2,), (BN,), ("conv", 32)) + HEAD, 2)
    assert convnet.plan((8, 8, 3), (("conv", 32), (DWS2,), ("bn_add_relu_down", 2)) + HEAD, 2)
    with pytest.raises(convnet.ConvNetError, match=r"-2: layer 2 \(RCN_HIPX_BN_ADD\): the skip's source, layer 0, has another output shape \(8x8x32, not 4x4x32\)"):
        convnet.plan((8, 8, 3), (("conv", 32), (DWS2,), (BNA, 2), ("conv", 32)) + HEAD, 2)
    # bn / bn_add as a skip's source for every kind that adds a skip; bn_add whose source is a bn_relu, a pool, a bn, a bn_add
    for src in (((PW, 32), (BN,)), ((PW, 32), (BNA, 2))):
        for add in (("bn_add_relu", 2), (BNA, 2)):
            assert convnet.plan((8, 8, 3), STEM + src + ((PW, 32), add, ("conv", 32)) + HEAD, 2)
        assert convnet.plan((8, 8, 3), STEM + src + (("conv_linear_s2", 32), ("bn_add_relu_down", 2)) + HEAD, 2)
    for front in (STEM, (("conv", 32), ("pool",)), STEM + ((PW, 32), (BN,)), STEM + ((PW, 32), (BNA, 2))):
        assert convnet.plan((8, 8, 3), front + ((PW, 32), (BNA, 2), ("conv", 32)) + HEAD, 2)


# ---- plan text ------------------------------------------------------------------------------------------------------------------------------

def _plan(convnet, monkeypatch, spec, precision="fp32", **env):
    for k, v in env.items():
        monkeypatch.setenv("RCN_HIPX_" + k.upper(), str(v))
    lines = plan_lines(convnet.plan(spec[0], spec[1], spec[2], precision))
    for k in env:
        monkeypatch.delenv("RCN_HIPX_" + k.upper())
    return lines


TILES = re.compile(r"tiles of (\d+) (?:output|block) rows x 256 (?:pieces of 16 bytes|blocks) \((\d+) bands x (\d+) slabs per image, (\d+) tiles\), workgroups (.*)$")
CHUNKS = re.compile(r"(\d+) channel groups x (\d+) chunks of (\d+) output pixels$")


def _tiles(line):
    th, bands, slabs, items, grid = TILES.search(line).groups()
    return int(th), int(bands), int(slabs), int(items), grid


@pytest.mark.parametrize("precision", ["fp32", "bf16"])
@pytest.mark.parametrize("name", sorted(NETS))
def test_every_strided_depthwise_layer_has_its_lines_and_computes_in_fp32(convnet, monkeypatch, name, precision):
    """forward, input gradient (none for layer 0) and weight gradient per strided layer, the same lines in both precision modes (fp32
    arithmetic by kind, no operand copy); evaluation: the forward lines alone; the bucket plan carries them too"""
    spec = NETS[name]
    n_s2, first = sum(l[0] == DWS2 for l in spec[1]), spec[1][0][0] == DWS2
    lines = _plan(convnet, monkeypatch, spec, precision)
    got, wg = _s2(lines), _wg(lines)
    assert len(got) == 2 * n_s2 - first and sum("k_dw_s2_fwd" in l for l in got) == n_s2 == len(wg), got
    assert all("(fp32 arithmetic)" in l and TILES.search(l) for l in got) and all("k_dw_s2_wgrad (fp32 arithmetic)" in l and CHUNKS.search(l) for l in wg), got + wg
    assert got + wg == _s2(_plan(convnet, monkeypatch, spec, "fp32")) + _wg(_plan(convnet, monkeypatch, spec, "fp32")), "the kind's lines depend on the precision mode"
    ev = _s2(plan_lines(convnet.plan_eval(spec[0], spec[1], spec[2], precision)))
    assert len(ev) == n_s2 and all("k_dw_s2_fwd" in l for l in ev), ev
    bucket = [l.strip() for l in convnet.plan(spec[0], spec[1], spec[2], precision, buckets=0).splitlines()]
    assert _s2(bucket) == got and _wg(bucket) == wg, bucket


def test_bf16_mode_makes_no_operand_copies_of_a_strided_depthwise_layer(convnet):
    """16 GEMM layers behind layer 0 and a strided depthwise layer still prepare their copies in one launch: the kind is not counted"""
    def layers(dense):
        return (("conv", 32), (DWS2,), ("bn_relu",)) + (("dense_relu", 32),) * (dense - 1) + (("dense", 4),)
    lines = plan_lines(convnet.plan((4, 4, 3), layers(16), 2, "bf16"))
    assert lines[0].startswith("bf16 operand copies of every layer's weights, both orientations: k_prep_all_bf16 (one launch)"), lines[0]
    lines = plan_lines(convnet.plan((4, 4, 3), layers(17), 2, "bf16"))
    assert lines[0].startswith("bf16 operand copies: none prepared (17 matrix layers behind layer 0, one launch takes 16)"), lines[0]


def test_forms_the_gpu_cases_reach(convnet, monkeypatch):
    """From the plan lines, what each GPU case's comment names.  a: a 2 x 3 output, epilogue 3.  b / bh / bw: a 1 x 1, 1 x 4 and 4 x 1
    output above a pool, epilogue 0.  c: 24 quads (256 % 24 != 0), 10 x 24 = 240 pieces in one slab, three chunks of 128 output pixels over
    M_out = 300 (the last of 44) x three channel groups.  d: layer 0 without an input gradient, three bands x two slabs; at C = 256 two
    bands (10 = 8 + 2 output rows) x five slabs (1152 = 4 x 256 + 128 pieces), twelve chunks over M_out = 1440 (the last of 32) x eight
    groups; under halo_f32_slots = 3 three workgroups loop over the tiles."""
    a = _s2(_plan(convnet, monkeypatch, NETS["a"]))
    assert [l.split(" (fp32")[0] for l in a] == ["dwconv 3x3/2 4x6x32->2x3x32 epi 1: k_dw_s2_fwd", "dgrad dwconv 3x3/2 2x3x32->4x6x32 epi 3: k_dw_s2_dgrad<3>"], a
    assert all(_tiles(l)[:4] == (8, 1, 1, 3) for l in a), a
    for name, (h, w) in (("b", (2, 2)), ("bh", (2, 8)), ("bw", (8, 2))):
        got = _s2(_plan(convnet, monkeypatch, NETS[name]))
        assert got[0].startswith(f"dwconv 3x3/2 {h}x{w}x32->{h // 2}x{w // 2}x32 epi 1:") and got[1].startswith(f"dgrad dwconv 3x3/2 {h // 2}x{w // 2}x32->{h}x{w}x32 epi 0:"), got
    assert OPTIONS["c"] == (("pix_per_chunk", 128),)
    c = _plan(convnet, monkeypatch, NETS["c"], pix_per_chunk=128)
    assert [l.split(": k_dw")[0] for l in _s2(c)] == ["dwconv 3x3/2 12x20x96->6x10x96 epi 1", "dgrad dwconv 3x3/2 6x10x96->12x20x96 epi 3"] and all(_tiles(l)[:4] == (8, 1, 1, 5) for l in _s2(c)), _s2(c)
    assert 256 % (96 // 4) != 0 and 10 * 96 // 4 == 240
    assert [CHUNKS.search(l).groups() for l in _wg(c)] == [("3", "3", "128")] and NETS["c"][2] * 6 * 10 == 300 == 2 * 128 + 44, _wg(c)
    for env in ({}, dict(LOOPING)):
        lines = _plan(convnet, monkeypatch, NETS["d"], **env)
        d = _s2(lines)
        assert [l.split(" epi")[0] for l in d] == ["dwconv 3x3/2 40x72x32->20x36x32", "dwconv 3x3/2 20x36x256->10x18x256", "dgrad dwconv 3x3/2 10x18x256->20x36x256"], d
        assert " epi 3: k_dw_s2_dgrad<3>" in d[2] and _tiles(d[0])[:4] == (8, 3, 2, 48) and all(_tiles(l)[:4] == (8, 2, 5, 80) for l in d[1:]), d
        assert 10 % 8 != 0 and 10 > 8 and (18 * 256 // 4) % 256 != 0 and 18 * 256 // 4 > 256
        want = "3 looping over the tiles" if env else "a resident grid looping over the tiles"
        assert all(_tiles(l)[4] == want for l in d), d
        assert [CHUNKS.search(l).groups() for l in _wg(lines)] == [("8", "12", "128"), ("1", "45", "128")] and NETS["d"][2] * 10 * 18 == 1440 == 11 * 128 + 32, _wg(lines)


def _check_gating(convnet, spec, precision, buckets):
    """the gating table of the linear kinds, from the plan text of one net"""
    layers = spec[1]
    text = convnet.plan(spec[0], spec[1], spec[2], precision, buckets=0) if buckets else convnet.plan(spec[0], spec[1], spec[2], precision)
    lines = [l.strip() for l in text.splitlines()[1:] if l.strip()]
    bn_at = [i for i in range(len(layers) - 1, -1, -1) if layers[i][0] in ("bn_relu", "bn_add_relu", "bn_add_relu_down", BN, BNA)]
    red = [k for k, x in enumerate(lines) if x.startswith("bn-bwd-reduce")]      # in walk order: from the last layer down
    assert len(red) == len(bn_at), (len(red), bn_at)
    for i, k in zip(bn_at, red):
        l, linear = lines[k], layers[i][0] in (BN, BNA)
        assert l.endswith("; linear: no gate") == linear and ("gated by" in l or "gates itself" in l) == (not linear), (i, layers[i], l)
        if linear:
            # the input-gradient launch of the convolution above runs epilogue 0: the nearest line in front that is no weight gradient,
            # skip's add or bucket line
            back = [x for x in lines[:k] if x.startswith(("conv", "dwconv", "dgrad"))][-1]
            assert " epi 0:" in back, (i, back)
    # every skip's add: directly behind the input gradient of the layer above the source, in front of that layer's weight gradient
    adds = {s: i for i, l in enumerate(layers) if l[0] in ("bn_add_relu", BNA) for s in [i - l[1]]}
    at = [k for k, x in enumerate(lines) if x.startswith("skip-bwd")]
    assert len(at) == len(adds), (at, adds)
    for k in at:
        src = int(re.search(r"into layer (\d+)'s gradient", lines[k]).group(1))
        add, kind = layers[adds[src]][0], layers[src][0]
        self_words = "ungated: the sum has no ReLU behind it" if add == BNA else "gated "
        src_words = {"pool": f"ungated: layer {src} is a pool", BN: f"ungated: layer {src} is a batch normalisation without a ReLU",
                     BNA: f"ungated: layer {src} is a batch normalisation without a ReLU"}.get(kind, f"then gated by layer {src}'s output")
        assert f"(the skip's gradient {self_words}" in lines[k] and lines[k].endswith(src_words + ")"), lines[k]
        assert lines[k - 1].startswith(("conv", "dwconv", "dgrad")) and (" epi 3:" if kind in ("bn_relu", "conv", "bn_add_relu") else " epi 0:") in lines[k - 1], lines[k - 1:k + 1]
        assert lines[k + 1].startswith("wgrad"), lines[k:k + 2]
    return len(at)


@pytest.mark.parametrize("precision", ["fp32", "bf16"])
@pytest.mark.parametrize("name", sorted(NETS))
def test_the_gating_table_of_the_linear_kinds_from_the_plan(convnet, name, precision):
    """net e: bn_add from a bn_relu source and from a bn_add source, and a bn below a 1x1 convolution; net f: bn_add from a pool source,
    bn_add and bn below a ReLU convolution, bn below a depthwise layer -- in the step's plan and in the bucket plan at 0 bytes"""
    for buckets in (False, True):
        adds = _check_gating(convnet, NETS[name], precision, buckets)
        assert adds == {"e": 2, "f": 1}.get(name, 0)


def test_the_four_source_kinds_of_bn_add(convnet):
    """bn_relu, pool, bn, bn_add: the skip-bwd line's gate pair for each (the check of _check_gating on four small nets)"""
    for front in (STEM, (("conv", 32), ("pool",)), STEM + ((PW, 32), (BN,)), STEM + ((PW, 32), (BNA, 2))):
        spec = ((8, 8, 3), front + ((PW, 32), (BNA, 2), ("conv", 32)) + HEAD, 2)
        assert _check_gating(convnet, spec, "fp32", False) == (2 if front[-1][0] == BNA else 1)
    # ... and a linear source under the older adding kinds: ungated by the source, gated at the sum
    for add in (("bn_add_relu", 2),):
        spec = ((8, 8, 3), STEM + ((PW, 32), (BN,), (PW, 32), add, ("conv", 32)) + HEAD, 2)
        lines = plan_lines(convnet.plan(*spec))
        k, = [i for i, l in enumerate(lines) if l.startswith("skip-bwd")]
        assert "gated by the convolution above; ungated: layer 3 is a batch normalisation without a ReLU)" in lines[k], lines[k]


def _mbv2():
    inv = lambda c, co, s2: ((PW, 6 * c), ("bn_relu",), (DWS2,) if s2 else (DW,), ("bn_relu",), (PW, co), (BN,) if s2 or co != c else (BNA, 6))
    return STEM + STEM + inv(32, 32, False) + inv(32, 64, True) + inv(64, 64, False) + inv(64, 128, True) + ((PW, 256), ("bn_relu",), ("global_avgpool",), ("dense", 10))


def test_cifar_mbv2_plans_and_lists_31_reduction_jobs(convnet, monkeypatch):
    import bench_convnet
    in_shape, layers, B = bench_convnet.CONFIGS["cifar_mbv2"]
    assert (in_shape, B) == ((32, 32, 3), 512) and tuple(layers) == _mbv2() and sum(l[0] not in ("pool", "global_avgpool") for l in layers) == 31
    assert [i - l[1] for i, l in enumerate(layers) if l[0] == BNA] == [3, 15] and layers[3] == ("bn_relu",) and layers[15] == (BN,)
    for precision in ("fp32", "bf16"):
        lines = _plan(convnet, monkeypatch, (in_shape, layers, B), precision)
        assert lines[-1].startswith("update: k_reduce_all,") and " 31 layers' slabs in one launch" in lines[-1], lines[-1]
        got = _s2(lines)
        assert [l.split(" epi")[0] for l in got] == ["dwconv 3x3/2 32x32x192->16x16x192", "dwconv 3x3/2 16x16x384->8x8x384", "dgrad dwconv 3x3/2 8x8x384->16x16x384",
                                                     "dgrad dwconv 3x3/2 16x16x192->32x32x192"], got
        # whole-height bands at the benchmark's batch: 512 images x 3 slabs = 1536 tiles
        assert [_tiles(l)[:4] for l in got] == [(16, 1, 3, 1536), (8, 1, 3, 1536), (8, 1, 3, 1536), (16, 1, 3, 1536)], got
        assert _check_gating(convnet, (in_shape, layers, B), precision, False) == 2 == _check_gating(convnet, (in_shape, layers, B), precision, True)


# ---- FLOP count, HBM floor, state layout ------------------------------------------------------------------------------------------------------

def test_hbm_floor_by_hand_on_two_nets(convnet):
    """the strided layer: input map and output map read / written per pass as any convolution, 10 C parameters; bn as bn_relu, bn_add as
    bn_add_relu"""
    floor = convnet.ConvNet.step_hbm_floor_bytes
    mk = lambda in_shape, layers: type("N", (), {"in_shape": in_shape, "layers": [tuple(l) for l in layers]})()
    B = 2
    a = floor(mk((8, 8, 32), ((DWS2,), ("bn_relu",), ("dense", 4))), B)
    i, o = 8 * 8 * 32 * 4, 4 * 4 * 32 * 4
    hand = B * 2 * (i + o) + 3 * 10 * 32 * 4 + B * 7 * o + B * 3 * (o + 4 * 4) + 3 * (4 * 4 * 32 * 4 + 4) * 4
    assert a == hand, (a, hand)
    # the second net by hand: a first ReLU convolution (two passes), a 1x1 layer, bn_add (bn_relu's 7 maps, the skip read once more, the add
    # pass's three), a ReLU convolution and a dense layer on the flattened map; m: one 8 x 8 x 32 map in bytes
    m, w3, w1 = 8 * 8 * 32 * 4, 9 * 32 * 32 + 32, 32 * 32 + 32
    b = floor(mk((8, 8, 32), (("conv", 32), (PW, 32), (BNA, 2), ("conv", 32), ("dense", 4))), B)
    hand = (B * 4 * m + 3 * w3 * 4) + (B * 6 * m + 3 * w1 * 4) + B * 11 * m + (B * 6 * m + 3 * w3 * 4) + (B * 3 * (m + 4 * 4) + 3 * (8 * 8 * 32 * 4 + 4) * 4)
    assert b == hand, (b, hand)
    # ... and the linear kinds count as their ReLU kinds do
    lin = floor(mk((8, 8, 3), STEM + ((PW, 32), (BNA, 2), ("conv", 32), (PW, 32), (BN,), ("conv", 32)) + HEAD), B)
    rel = floor(mk((8, 8, 3), STEM + ((PW, 32), ("bn_add_relu", 2), ("conv", 32), (PW, 32), ("bn_relu",), ("conv", 32)) + HEAD), B)
    assert lin == rel


def test_state_layout_stays_version_1_and_carries_the_kinds(convnet):
    in_shape, layers, _ = NETS["e"]
    d = convnet.state_layout(in_shape, layers)
    assert (convnet.KIND[BN], convnet.KIND[BNA], convnet.KIND[DWS2]) == (12, 13, 14) and d.version == 1
    assert [d.layers[i].kind for i in range(d.n_layers)] == [convnet.KIND[l[0]] for l in layers]
    assert (d.layers[7].kind, d.layers[7].out) == (13, 6) and (d.layers[16].kind, d.layers[16].out) == (14, 64) and (d.layers[19].kind, d.layers[19].out) == (12, 32)
    resolved = [(l[0], 64) if l[0] in (DW, DWS2) else tuple(l) for l in layers]
    assert d.shape_and_layers() == (in_shape, resolved)
    sl = tensor_slices(in_shape, layers)
    with_params = [i for i, l in enumerate(layers) if l[0] not in ("pool", "global_avgpool")]
    assert d.n_log == n_logical(in_shape, layers) and [d.layer_off[i] for i in with_params] == [s[0].start for s in sl]
    assert param_shapes(in_shape, layout(layers))[with_params.index(16)] == (9, 64)
    body = np.zeros(int(d.body_bytes), dtype=np.uint8)
    d2, _, extra = convnet.read_state_file(convnet.write_state_file(d, body, b"x"))
    assert d2.shape_and_layers() == (in_shape, resolved) and extra == b"x"


# ---- the twin, pinned by plain loops ----------------------------------------------------------------------------------------------------------

def _hand_s2(x, W, b):
    """y[n][i][j][c] = b[c] + sum over kh, kw of W[3 kh + kw][c] x[n][2i + kh - 1][2j + kw - 1][c], zero outside the map: plain loops"""
    N, H, Wd, C = x.shape
    y = np.zeros((N, H // 2, Wd // 2, C))
    for n in range(N):
        for i in range(H // 2):
            for j in range(Wd // 2):
                acc = b.copy()
                for kh in range(3):
                    for kw in range(3):
                        hh, ww = 2 * i + kh - 1, 2 * j + kw - 1
                        if 0 <= hh < H and 0 <= ww < Wd:
                            acc += W[3 * kh + kw] * x[n, hh, ww]
                y[n, i, j] = acc
    return y


def test_twin_strided_depthwise_convolution_on_a_hand_computed_case():
    """Two samples of a 4 x 6 x 32 map.  Under L = sum v . z: dx[n][r][s] = sum over the (i, kh), (j, kw) with 2i + kh - 1 = r, 2j + kw - 1 = s
    of W[3 kh + kw] v[n][i][j]; dW[t] = sum over output pixels of x[2i + kh - 1][2j + kw - 1] v[i][j]; db = sum v -- all by plain loops"""
    C = 32
    rng = np.random.default_rng(0)
    x, v = rng.standard_normal((2, 4, 6, C)), rng.standard_normal((2, 2, 3, C))
    W, b = rng.standard_normal((9, C)) * 0.3, rng.standard_normal(C)
    layers = ((DWS2,), ("bn_relu",), ("dense", 1))
    flat = np.concatenate([W.ravel(), b, np.ones(C), np.zeros(C), np.zeros(2 * 3 * C), [0.0]])
    net = MbNet((4, 6, C), layers, flat)
    net.forward(x, False)
    z = net.outs[0]
    assert tuple(z.shape) == (2, C, 2, 3)
    assert np.allclose(z.detach().numpy().transpose(0, 2, 3, 1), _hand_s2(x, W, b), rtol=0, atol=1e-12)
    for m in net.mods:
        m.zero_grad()
    t = net.torch.from_numpy(np.ascontiguousarray(x.transpose(0, 3, 1, 2))).requires_grad_(True)
    (net._conv(net.mods[0], t) * net.torch.from_numpy(np.ascontiguousarray(v.transpose(0, 3, 1, 2)))).sum().backward()
    dx, dW = np.zeros_like(x), np.zeros((9, C))
    for i in range(2):
        for j in range(3):
            for kh in range(3):
                for kw in range(3):
                    r, s = 2 * i + kh - 1, 2 * j + kw - 1
                    if 0 <= r < 4 and 0 <= s < 6:
                        dx[:, r, s] += W[3 * kh + kw] * v[:, i, j]
                        dW[3 * kh + kw] += (x[:, r, s] * v[:, i, j]).sum(0)
    assert np.allclose(t.grad.numpy().transpose(0, 2, 3, 1), dx, rtol=0, atol=1e-12)
    g = net._flat(lambda p: p.grad if p.grad is not None else net.torch.zeros_like(p))
    ws, bs = tensor_slices((4, 6, C), layers)[0]
    assert np.allclose(g[ws].reshape(9, C), dW, rtol=0, atol=1e-12) and np.allclose(g[bs], v.sum((0, 1, 2)), rtol=0, atol=1e-12)
    # the four parity classes of the library's input gradient are this sum: 1 / 2 / 2 / 4 taps per class
    taps = np.zeros((4, 6), dtype=int)
    for i in range(2):
        for j in range(3):
            for kh in range(3):
                for kw in range(3):
                    if 0 <= 2 * i + kh - 1 < 4 and 0 <= 2 * j + kw - 1 < 6:
                        taps[2 * i + kh - 1, 2 * j + kw - 1] += 1
    assert taps[0, 0] == 1 and taps[0, 1] == 2 and taps[1, 0] == 2 and taps[1, 1] == 4 and taps[3, 5] == 1 and taps[3, 4] == 1 and taps[2, 5] == 1, taps
    # the bf16 twin does not round this layer's operands
    r = MbNet((4, 6, C), layers, flat, operand="bf16")
    r.forward(x, False)
    assert np.array_equal(r.outs[0].detach().numpy(), z.detach().numpy())


def test_twin_bn_add_forward_and_backward_on_a_hand_computed_case():
    """y = gamma (z - mean) / sqrt(var + eps) + beta + s on the running statistics, no activation: under L = sum v . y the gradient of z is
    v gamma / sqrt(var + eps) and the gradient of the source is v wherever -- also where y or s is negative"""
    import torch
    C = 32
    rng = np.random.default_rng(3)
    in_shape, layers = (2, 3, C), ((PW, C), ("bn_relu",), (PW, C), (BNA, 2), ("conv", C), ("dense", 1))
    flat = random_params(rng, in_shape, layers)
    net = MbNet(in_shape, layers, flat)
    mean, var = rng.standard_normal(C) * 0.1, 1.0 + 0.2 * rng.random(C)
    net.set_bn_stats(np.concatenate([np.zeros(C), np.ones(C), mean, var]))
    x, v = rng.standard_normal((2,) + in_shape), rng.standard_normal((2, 2, 3, C))
    net.forward(x, False)
    s, z, y = (net.outs[i] for i in (1, 2, 3))
    gamma, beta = (flat[t].astype(np.float64) for t in tensor_slices(in_shape, layers)[3])
    nhwc = lambda t: t.detach().numpy().transpose(0, 2, 3, 1)
    want = gamma * (nhwc(z) - mean) / np.sqrt(var + 1e-5) + beta + nhwc(s)
    assert np.allclose(nhwc(y), want, rtol=0, atol=1e-12) and (want < 0).mean() > 0.2, "no ReLU: negative values pass"
    gz, gs = torch.autograd.grad((y * torch.from_numpy(np.ascontiguousarray(v.transpose(0, 3, 1, 2)))).sum(), (z, s), retain_graph=True)
    assert np.allclose(nhwc(gz), v * gamma / np.sqrt(var + 1e-5), rtol=0, atol=1e-12)
    # the source's gradient: the skip's share v itself, plus the path through layer 2's convolution -- take the share alone
    net2 = MbNet(in_shape, layers, flat, drop_skip_share=True)
    net2.set_bn_stats(np.concatenate([np.zeros(C), np.ones(C), mean, var]))
    net2.forward(x, False)
    gs2, = torch.autograd.grad((net2.outs[3] * torch.from_numpy(np.ascontiguousarray(v.transpose(0, 3, 1, 2)))).sum(), (net2.outs[1],))
    assert np.allclose(nhwc(gs) - nhwc(gs2), v, rtol=0, atol=1e-12)


def _share(got, ref, in_shape, layers, rtol):
    """the worst |d| / allowance of close_per_tensor, without asserting"""
    worst = 0.0
    for ws, bs in tensor_slices(in_shape, layers):
        for t in (ws, bs):
            worst = max(worst, float(np.abs(got[t] - ref[t]).max()) / (rtol * max(1e-3, float(np.abs(ref[t]).max())) + 1e-6))
    return worst


# two inverted residual blocks on a 4 x 6 map -- the second's source is the first's bn_add -- and a strided block behind them
HAND = ((4, 6, 32), ((PW, 32), ("bn_relu",)) + inverted(32) + inverted(32) + inverted_s2(32, 32) + (("conv", 32), ("dense", 3)), 2)
MUTANTS = ["phase_off", "taps_unreversed", "taps_transposed", "relu_in_bn", "gate_linear", "gate_linear_source", "drop_skip_share"]


@pytest.mark.parametrize("mutant", MUTANTS)
def test_the_twin_sees_each_mutant(mutant):
    """Each mutant moves the twin's gradient by more than an fp32 allowance (2e-4 of a tensor's scale + 1e-6) of _twin_checks.compare on a
    two-sample 4 x 6 x 32 case, by a wide margin (printed).  The gradient is taken on the running statistics (mean 0, variance 1), as the
    depthwise file takes it."""
    import torch
    in_shape, layers, B = HAND
    flat = random_params(np.random.default_rng(0), in_shape, layers)
    rng = np.random.default_rng(1)
    x, y = rng.standard_normal((B,) + in_shape), rng.integers(0, 3, B)

    def grad(**kw):
        net = MbNet(in_shape, layers, flat, **kw)
        for m in net.mods:
            m.zero_grad()
        torch.nn.functional.cross_entropy(net.forward(x, False), torch.from_numpy(y.astype(np.int64))).backward()
        return net._flat(lambda p: p.grad if p.grad is not None else torch.zeros_like(p))
    share = _share(grad(**{mutant: True}), grad(), in_shape, layers, RTOL["fp32"])
    print(f"{mutant}: the gradient moves by {share:.0f} allowances")
    assert share > 10.0, (mutant, share)


# ---- the conditions the GPU comparison rests on, from the twin alone ------------------------------------------------------------------------

@pytest.mark.parametrize("precision", ["fp32", "bf16"])
@pytest.mark.parametrize("name", sorted(NETS))
def test_margin_condition_of_the_comparison_holds(name, precision):
    """_twin_checks.compare asserts margin > 4 * rtol2 * scale before it compares the correct count: at the seeds in use, from the twin alone"""
    in_shape, layers, _ = NETS[name]
    flat, x, y = case(name)
    ref = twin_schedule(MbNet(in_shape, layers, flat, operand="bf16" if precision == "bf16" else "f64"), x, y, STEPS)
    print(f"net {name} {precision} seeds {SEEDS[name]}: margin {ref['margin']:.4f}, scale {ref['scale']:.3f}, bound {4 * RTOL_2[precision] * ref['scale']:.4f}")
    assert ref["margin"] > 4 * RTOL_2[precision] * ref["scale"], (name, precision, ref["margin"], ref["scale"])


@pytest.mark.parametrize("name", sorted(NETS))
def test_bf16_twin_agrees_with_itself_in_float32(name):
    """The reference's own error, as tests/test_convnet_pw_plan.py measures it: the bf16-operand twin evaluated in float32 stays within
    0.3 of every bf16 allowance of the comparison the GPU test makes against the same twin in float64."""
    in_shape, layers, _ = NETS[name]
    flat, x, y = case(name)
    ref = twin_schedule(MbNet(in_shape, layers, flat, operand="bf16"), x, y, STEPS)
    f32 = twin_schedule(MbNet(in_shape, layers, flat, operand="bf16", arithmetic="float32"), x, y, STEPS)
    with contextlib.redirect_stdout(io.StringIO()):
        share = compare(NETS[name], f32, ref, RTOL["bf16"], RTOL_2["bf16"], STEPS, f"net {name} twin in float32")
    print(f"net {name}: the bf16 twin in float32 against itself in float64: worst share of an allowance = {share:.3f}")
    assert share < 0.3, (name, share)


def test_the_exact_net_is_exact_in_every_precision():
    """tests/_mb_ref.py's small-integer net: every operand is an integer of at most 8 bits (exact in bf16), every sum below 2^24 (exact in
    float32 in any order), negative values pass the linear batch normalisation, and the twin's float64 evaluation on the running
    statistics gives NumPy's integers"""
    flat, stats, x, want, a1, a2 = exact_case()
    assert np.abs(x).max() <= 2 and (a1 < 0).mean() > 0.2 and a2.max() <= 255 and np.abs(want).max() < 2 ** 24
    for ws, _ in tensor_slices(X_SPEC[0], X_SPEC[1])[0:3:2]:
        assert set(np.unique(flat[ws])) <= {-1.0, 0.0, 1.0}
    net = MbNet(X_SPEC[0], X_SPEC[1], flat)
    net.set_bn_stats(stats)
    z = net.logits(x, train=False)
    assert np.array_equal(np.rint(z), want) and np.abs(z - want).max() < 1e-3 * max(1.0, np.abs(want).max())
