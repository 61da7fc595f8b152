"""Without a GPU, what tests/test_gpu_convnet_kinds_forms.py rests on (the table: tests/_kinds_cases.py).  From the plan's own text: that each
case reaches the form its comment names -- the band heights, bands, slabs and tiles of k_dw, the looping grid on which a lane's quad
changes with every tile, the edges of select_dw (kDwMinTiles, th < H + 8), the weight gradient's chunks, the NT of every k_pw launch, the
slices at the LDS limit and the fall-back one width further, the launch in front of each skip-bwd line, the smallest maps -- and that every
NT in 1 .. 8 and every band height in {8, 16, 32} is planned by some case.  From the twin alone: the margin condition of
tests/_twin_checks.py's comparison per net and precision, the bf16 twin agreeing with itself in float32, no ReLU pre-activation of the
tall-band nets within 1e-6 of zero (for the wide ones on the parameters with the table's NUDGES), and the fp32 twin agreeing with itself
in float32 where sums are long or batch normalisation has two rows.  Three mutants of the twin (a band that reads its upper halo row as
zeros, a weight cache not keyed by the quad, two accumulator tiles stored in each other's place) each move the comparison's quantities by more than an allowance on the case that is there for them.  The
small-integer nets at the wide shapes are exact."""
import contextlib
import functools
import io
import re

import numpy as np
import pytest
from _convnet_util import convnet_loaded, plan_lines  # noqa: F401  (fixture)
from _dw_ref import RTOL, RTOL_2, STEPS, DwNet, compare, exact_case, tensor_slices
from _kinds_cases import (CHUNK_FORMULA, DW_CHUNKS, DW_TILES, EXACT, EXACT_RUNS, LARGE, LOOPING, NETS, NUDGES, PW0, PW1, PW_NT, RUNS, SEEDS, TIE, TWIN_F32_DISTANCE, KindsNet, case,
                          twin)
from _twin_checks import twin_schedule

TILES = re.compile(r"tiles of (\d+) rows x 256 pieces of 16 bytes \((\d+) bands x (\d+) slabs per image, (\d+) tiles\), workgroups (.*)$")
CHUNKS = re.compile(r"(\d+) channel groups x (\d+) chunks of (\d+) pixels$")
NT = re.compile(r"k_pw<(f32|bf16), (\d)>")
RESIDENT = "a resident grid looping over the tiles"


def _plan(convnet, monkeypatch, spec, precision="fp32", options=()):
    for k, v in options:
        monkeypatch.setenv("RCN_HIPX_" + k.upper(), str(v))
    lines = plan_lines(convnet.plan(spec[0], spec[1], spec[2], precision))
    for k, _ in options:
        monkeypatch.delenv("RCN_HIPX_" + k.upper())
    return lines


def _dw(lines):
    return [l for l in lines if l.startswith("dwconv")]


def _wg(lines):
    return [l for l in lines if l.startswith("wgrad dwconv")]


def _pw(lines):
    return [l for l in lines if l.startswith("conv1x1")]


def _tiles(line):
    th, bands, slabs, items, grid = TILES.search(line).groups()
    return (int(th), int(bands), int(slabs), int(items)), grid


# ---- k_dw ------------------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", sorted(DW_TILES))
def test_depthwise_nets_plan_their_band_form(convnet, monkeypatch, name):
    """forward as layer 0, forward and gated input gradient in the tiles the table names, in both precisions (fp32 arithmetic by kind); the
    weight gradient's chunks over M pixels under the run's options"""
    spec = NETS[name]
    H, W, C = spec[0]
    runs = [r for r in RUNS if r[0] == name]
    assert runs
    for _, precision, options in runs:
        lines = _plan(convnet, monkeypatch, spec, precision, options)
        d = _dw(lines)
        assert [l.split(":")[0] for l in d] == [f"dwconv 3x3 {H}x{W}x{C} epi {e}" for e in (1, 1, 3)] and "k_dw<3>" in d[2], d
        assert all(_tiles(l)[0] == DW_TILES[name] for l in d), d
        assert all(_tiles(l)[1] == ("3 looping over the tiles" if options == LOOPING else RESIDENT) for l in d), d
        M, chunks, ppc = DW_CHUNKS[name]
        assert M == spec[2] * H * W and [CHUNKS.search(l).groups() for l in _wg(lines)] == [(str(C // 32), str(chunks), str(ppc))] * 2, _wg(lines)
        assert chunks == -(-M // ppc)
    th, bands, slabs, tiles = DW_TILES[name]
    assert bands == -(-H // th) and slabs == -(-(W * C // 4) // 256) and tiles == spec[2] * bands * slabs


def test_what_the_band_forms_are(convnet, monkeypatch):
    """bands16 / seam16: 20 = 16 + 4 rows, a seam and a partial last band.  band32 / whole32: one band of 32 rows on 28, taller than the
    map; band32's weight gradient by the default formula above the 128-pixel floor at the default options, whole32's under wg_target = 256
    (at the default the floor: 448 chunks of 128).  bands32 / seam32: 36 = 32 + 4.  bands16 and quads: 264 pieces per row = 256 + 8, 24
    quads, 256 % 24 = 16: on three workgroups each workgroup's consecutive tiles lie in different slabs, so its lanes' quads change with
    every tile."""
    for tall, narrow, th, bands, H in (("bands16", "seam16", 16, 2, 16 + 4), ("band32", "whole32", 32, 1, 28), ("bands32", "seam32", 32, 2, 32 + 4)):
        assert DW_TILES[tall] == (th, bands, 2, 1024) and DW_TILES[narrow] == (th, bands, 1, 1024) and NETS[tall][0][0] == NETS[narrow][0][0] == H
    assert ("band32", "fp32", ()) in RUNS and DW_CHUNKS["band32"][2] == 256 > 128
    assert ("whole32", "fp32", CHUNK_FORMULA) in RUNS and DW_CHUNKS["whole32"][2] == 256
    floor = _wg(_plan(convnet, monkeypatch, NETS["whole32"]))
    assert all(CHUNKS.search(l).groups() == ("1", "448", "128") for l in floor), floor
    for name in ("bands16", "quads"):
        H, W, C = NETS[name][0]
        th, bands, slabs, tiles = DW_TILES[name]
        assert W * C // 4 == 264 and 256 % (C // 4) == 16 and slabs == 2
        for b in range(3):
            mine = [item % slabs for item in range(b, tiles, 3)]
            assert len(mine) >= 2 and all(u != v for u, v in zip(mine, mine[1:])), (b, mine[:8])
        assert all((name, p, LOOPING) in RUNS for p in ("fp32", "bf16"))


def test_the_edges_of_the_band_selector(convnet, monkeypatch):
    """kDwMinTiles: one image fewer than 1024 tiles' worth plans bands of 8 rows, on the one-slab and on the two-slab net.  th < H + 8: at
    H = 24 a band of 32 rows is refused (16 is taken), at H = 25 it is taken."""
    in_shape, layers, B = NETS["seam16"]
    assert _tiles(_dw(_plan(convnet, monkeypatch, (in_shape, layers, B - 1)))[1])[0] == (8, 3, 1, 3 * (B - 1))
    assert _tiles(_dw(_plan(convnet, monkeypatch, ((24, 3, 32), layers, 1024)))[1])[0] == (16, 2, 1, 2048)
    assert _tiles(_dw(_plan(convnet, monkeypatch, ((25, 3, 32), layers, 1024)))[1])[0] == (32, 1, 1, 1024)
    in_shape, layers, B = NETS["bands16"]
    assert B == 256 and all(_tiles(l)[0] == (8, 3, 2, 1530) for l in _dw(_plan(convnet, monkeypatch, (in_shape, layers, 255))))


def test_the_integer_nets_plan_the_wide_band_forms(convnet, monkeypatch):
    """evaluation: two forward launches per net, in both precisions; bands16 on three looping workgroups too"""
    for name, options in EXACT_RUNS:
        in_shape, layers, B = EXACT[name]
        for precision in ("fp32", "bf16"):
            for k, v in options:
                monkeypatch.setenv("RCN_HIPX_" + k.upper(), str(v))
            ev = _dw(plan_lines(convnet.plan_eval(in_shape, layers, B, precision)))
            for k, _ in options:
                monkeypatch.delenv("RCN_HIPX_" + k.upper())
            assert len(ev) == 2 and all(" epi 1: k_dw<1>" in l and _tiles(l)[0] == DW_TILES[name] for l in ev), ev
            assert all(_tiles(l)[1] == ("3 looping over the tiles" if options else RESIDENT) for l in ev), ev
    assert all((EXACT[n][0], EXACT[n][2]) == (NETS[n][0], NETS[n][2]) for n in EXACT)


# ---- k_pw ------------------------------------------------------------------------------------------------------------------------------------

def _nt(lines, epi):
    return [int(NT.search(l).group(2)) for l in _pw(lines) if f" epi {epi}:" in l]


@pytest.mark.parametrize("precision", ["fp32", "bf16"])
def test_the_chain_plans_every_untested_instantiation(convnet, monkeypatch, precision):
    """pw = 1: NT = 6, 2, 7, 2, 5, 3, 1 forward and 3, 5, 2, 7, 2, 6 in the gated input gradients, each over M = 175 rows = one full and one
    partial row block, K-tile counts 1, 2, 3, 5, 6, 7 (no power of two but 1 and 2), the input read once; pw = 0: the implicit GEMM, its
    32-wide column blocks reading the input 3, 5 and 7 times"""
    spec = NETS["chain"]
    assert spec[2] * spec[0][0] * spec[0][1] == 175 == 128 + 47
    lines = _plan(convnet, monkeypatch, spec, precision, PW1)
    assert (_nt(lines, 1), _nt(lines, 3)) == PW_NT["chain"], _pw(lines)
    assert all(f"k_pw<{'bf16' if precision == 'bf16' else 'f32'}, " in l and ", 2 row blocks of 128 rows on a resident grid, input read once" in l for l in _pw(lines)), _pw(lines)
    ks = {int(re.search(r"weights \[(\d+)\]", l).group(1)) // 32 for l in _pw(lines)}
    assert ks == {1, 2, 3, 5, 6, 7}, ks
    lines = _plan(convnet, monkeypatch, spec, precision, PW0)
    assert len(_pw(lines)) == 13 and not any("k_pw<" in l for l in lines)
    reads = {int(re.search(r"input read (\d+) times", l).group(1)) for l in _pw(lines) if "32-wide column blocks" in l}
    assert {3, 5, 7} <= reads, _pw(lines)


def test_the_slice_limit_and_the_first_width_past_it(convnet, monkeypatch):
    """[512][32] fp32 is 512 x (32 + 8) x 4 bytes = exactly 80 KB of dynamic LDS, the largest request of the launcher; [1024][32] bf16;
    NT = 8 in two and in four column slices; the 544- and 1056-deep contractions (forward and input gradient) on the implicit GEMM with
    split-K although pw = 1"""
    assert 512 * (32 + 8) * 4 == 80 * 1024
    for name, precision, K, slices, word in (("limit32", "fp32", 512, 2, "f32"), ("limit16", "bf16", 1024, 4, "bf16")):
        assert (name, precision, PW1) in RUNS
        got = _pw(_plan(convnet, monkeypatch, NETS[name], precision, PW1))
        assert len(got) == 7, got
        assert f"k_pw<{word}, 8>, weights [32][256] staged once" in got[0] and got[0].endswith(f"input read {slices} times ({slices} column slices)"), got[0]
        assert f"->64 epi 1: k_pw<{word}, 1>, weights [{K}][32] staged once" in got[1] and got[1].endswith("input read 2 times (2 column slices)"), got[1]
        past = [l for l in got if f"x{K + 32}->" in l]
        kernel = "k_conv_fwd_bf16<1, tile, " if precision == "bf16" else "k_conv_fwd<1, tile, "
        assert [l.split(":")[0][-5:] for l in past] == ["epi 1", "epi 3"] and all(kernel in l and "split-K" in l and "k_splitk_epilogue" in l for l in past), past
        assert f"k_pw<{word}, 8>, weights [64][256]" in got[-1] and " epi 3:" in got[-1], got[-1]


# ---- the kinds composed ----------------------------------------------------------------------------------------------------------------------

def _around_skips(lines):
    return [(lines[i - 1], lines[i], lines[i + 1]) for i, l in enumerate(lines) if l.startswith("skip-bwd")]


@pytest.mark.parametrize("precision", ["fp32", "bf16"])
def test_the_launch_in_front_of_each_skip_add(convnet, monkeypatch, precision):
    """neck: the 1x1 layer above the source (k_pw, or the implicit GEMM under pw = 0) writes all of the source's gradient, then
    k_skip_bwd_add_down, then that layer's weight gradient.  sepdown: k_dw<3> in front of k_skip_bwd_add_down.  sepdown2: both skip kernels,
    a depthwise layer on the strided layer's 4 x 6 map in front of k_skip_bwd_add"""
    for options, kernel in ((PW1, "k_pw<"), (PW0, "k_conv_fwd")):
        (before, add, after), = _around_skips(_plan(convnet, monkeypatch, NETS["neck"], precision, options))
        assert before.startswith("conv1x1 8x12x32->64 epi 3: " + kernel) and after.startswith("wgrad conv1x1 8x12x64->32"), (before, after)
        assert "k_skip_bwd_add_down" in add and "into layer 1's gradient" in add and "then gated by layer 1's output" in add, add
    (before, add, after), = _around_skips(_plan(convnet, monkeypatch, NETS["sepdown"], precision))
    assert before.startswith("dwconv 3x3 8x12x32 epi 3: k_dw<3>") and after.startswith("wgrad dwconv 3x3 8x12x32"), (before, after)
    assert "k_skip_bwd_add_down" in add and "into layer 1's gradient" in add, add
    first, second = _around_skips(_plan(convnet, monkeypatch, NETS["sepdown2"], precision, PW1))
    assert first[0].startswith("dwconv 3x3 4x6x64 epi 3: k_dw<3>") and "k_skip_bwd_add," in first[1] and "into layer 5's gradient" in first[1], first
    assert second[0].startswith("dwconv 3x3 8x12x32 epi 3: k_dw<3>") and "k_skip_bwd_add_down" in second[1] and "into layer 1's gradient" in second[1], second
    # in the bucket plan the add stays in the iteration of the layer above the source
    for name, options in (("neck", PW1), ("neck", PW0), ("sepdown", ())):
        for k, v in options:
            monkeypatch.setenv("RCN_HIPX_" + k.upper(), str(v))
        spec = NETS[name]
        lines = [l.strip() for l in convnet.plan(spec[0], spec[1], spec[2], precision, buckets=0).splitlines()]
        for k, _ in options:
            monkeypatch.delenv("RCN_HIPX_" + k.upper())
        i, = [k for k, x in enumerate(lines) if x.startswith("skip-bwd")]
        opened = [x for x in lines[:i] if x.startswith("bucket") and "done" not in x][-1]
        assert re.fullmatch(r"bucket \d+: layers 2 \.\. 2", opened), opened


def test_the_smallest_maps(convnet, monkeypatch):
    """2 x 2 -> 1 x 1: one output tile, one tile per parity class of the input gradient; a 1 x 1 depthwise map above a pool (epilogue 0);
    H = 1 and W = 1"""
    lines = _plan(convnet, monkeypatch, NETS["s2x2"])
    assert any(l.startswith("conv3x3/2 2x2x32->1x1x64 epi 1:") for l in lines), lines
    d, = [l for l in lines if l.startswith("dgrad conv3x3/2 1x1x64->2x2x32 epi 0:")]
    assert d.count(": 1 tiles") == 4 and any(l.startswith("skip-bwd 1x1x32: k_skip_bwd_add_down") for l in lines), lines
    d = _dw(_plan(convnet, monkeypatch, NETS["dw1x1"], options=PW1))
    assert [l[:25] for l in d] == ["dwconv 3x3 1x1x32 epi 1: ", "dwconv 3x3 1x1x32 epi 0: "] and "k_dw<0>" in d[1], d
    for name, shape in (("row", "1x5x32"), ("col", "5x1x32")):
        d = _dw(_plan(convnet, monkeypatch, NETS[name]))
        assert [l.split(":")[0] for l in d] == [f"dwconv 3x3 {shape} epi {e}" for e in (1, 1, 3)], d
    assert all((n, "fp32") in {(r[0], r[1]) for r in RUNS} for n in ("s2x2", "dw1x1", "row", "col"))


def test_every_nt_and_every_band_height_is_planned_by_some_case(convnet, monkeypatch):
    """over the runs of the table: k_pw<.., NT> for every NT in 1 .. 8 in both operand precisions, bands of 8, 16 and 32 rows"""
    nts, ths = {"f32": set(), "bf16": set()}, set()
    for name, precision, options in RUNS:
        lines = _plan(convnet, monkeypatch, NETS[name], precision, options)
        for l in _pw(lines):
            m = NT.search(l)
            if m:
                nts[m.group(1)].add(int(m.group(2)))
        ths |= {_tiles(l)[0][0] for l in _dw(lines)}
    assert nts == {"f32": set(range(1, 9)), "bf16": set(range(1, 9))} and ths == {8, 16, 32}, (nts, ths)


# ---- the premises of the comparison, from the twin alone -------------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def _schedule(name, precision, arithmetic="float64"):
    flat, x, y = case(name)
    return twin_schedule(twin(name, precision, flat, arithmetic=arithmetic), x, y, STEPS)


PAIRS = sorted({(r[0], r[1]) for r in RUNS})


@pytest.mark.parametrize("name,precision", PAIRS, ids=[f"{n}-{p}" for n, p in PAIRS])
def test_margin_condition_of_the_comparison_holds(name, precision):
    """_twin_checks.compare asserts margin > 4 * rtol2 * scale before it compares the correct count: at the seeds in use, from the twin alone"""
    ref = _schedule(name, precision)
    print(f"net {name} {precision} seeds {SEEDS[name]}: margin {ref['margin']:.4f}, scale {ref['scale']:.3f}, bound {4 * RTOL_2[precision] * ref['scale']:.4f}")
    assert ref["margin"] > 4 * RTOL_2[precision] * ref["scale"], (name, precision, ref["margin"], ref["scale"])


def _self_share(name, precision, **kw):
    with contextlib.redirect_stdout(io.StringIO()):
        return compare(NETS[name], _schedule(name, precision, "float32"), _schedule(name, precision), RTOL[precision], RTOL_2[precision], STEPS, f"net {name} twin in float32", **kw)


@pytest.mark.parametrize("name", sorted(n for n, p in PAIRS if p == "bf16"))
def test_bf16_twin_agrees_with_itself_in_float32(name):
    """The reference's own error: the bf16-operand twin evaluated in float32 stays within 0.3 of every bf16 allowance of the comparison the
    GPU test makes against the same twin in float64."""
    share = _self_share(name, "bf16")
    print(f"net {name}: the bf16 twin in float32 against itself in float64: worst share of an allowance = {share:.3f}")
    assert share < 0.3, (name, share)


@pytest.mark.parametrize("name", sorted(LARGE) + ["quads", "s2x2", "dw1x1"])
def test_fp32_twin_agrees_with_itself_in_float32(name):
    """The same for the unrounded twin at the fp32 bounds, where its own float32 run could come near them: weight gradients summed over
    30720 to 71680 pixels (more than any other twin case), and batch normalisation over the two rows of a 1 x 1 map at B = 2.  Every
    quantity stays within 0.3 of its allowance.  For the bias gradients of the wide nets' depthwise layers (zero in exact arithmetic,
    held at the floor scale) the table records the measured distance, TWIN_F32_DISTANCE: asserted here with a tenth on top (torch's float32 sums
    depend on its thread count), and the tensor is allowed the larger of the bound and four times the record -- in this test alone; the
    GPU comparison widens nothing, the device's sums leave these tensors within 0.03 of the unwidened allowance."""
    kw = {}
    if name in TWIN_F32_DISTANCE:
        ref, f32 = _schedule(name, "fp32"), _schedule(name, "fp32", "float32")
        sl = tensor_slices(NETS[name][0], NETS[name][1])
        allowance = RTOL["fp32"] * 1e-3 + 1e-6
        for li, recorded in TWIN_F32_DISTANCE[name].items():
            assert NETS[name][1][li][0] == "dwconv_linear" and np.abs(ref["grad"][sl[li][1]]).max() < 1e-12, "zero in exact arithmetic: the floor scale"
            d = float(np.abs(f32["grad"][sl[li][1]] - ref["grad"][sl[li][1]]).max())
            print(f"net {name} layer {li} bias gradient: float32 twin against float64 max |d| = {d:.3e} (recorded {recorded:.3e}) = {d / allowance:.2f} allowances")
            assert d <= 1.1 * recorded, (name, li, d, recorded)
        kw = dict(widened_gradients={(li, "biases"): max(1.0, 4 * recorded / allowance) for li, recorded in TWIN_F32_DISTANCE[name].items()})
    share = _self_share(name, "fp32", **kw)
    print(f"net {name}: the twin in float32 against itself in float64: worst share of an fp32 allowance = {share:.3f}")
    assert share < 0.3, (name, share)


@pytest.mark.parametrize("name", sorted(LARGE))
def test_no_relu_tie_within_float32_reach(name):
    """tests/test_convnet_stride_plan.py's rule for its net d: the device decides a gate on a float32 pre-activation a few 1e-7 off the
    twin's; no element of either ReLU map of a tall-band net is closer to zero than 1e-6, on the parameters as `case` returns them (for the
    wide nets: with NUDGES).  The error of a pre-activation near zero is that of a 10-term fp32 sum normalised by the channel's statistics
    and does not grow with the map's largest element; that one is bounded only to keep the maps ordinary (the 11.8 million elements of
    bands32 reach 17.8, the others stay below 14)"""
    import torch
    in_shape, layers, _ = NETS[name]
    flat, x, _ = case(name)
    net = DwNet(in_shape, layers, flat)
    assert all(layers[l] == ("bn_relu",) and 1 <= k <= 3 for (l, _), k in NUDGES.get(name, {}).items()), "a nudge is one to three steps of 1e-5 on a beta"
    with torch.no_grad():
        net.forward(x, True)
        for i in (1, 3):
            assert layers[i][0] == "bn_relu"
            pre = net.mods[i](net.outs[i - 1]).numpy()
            print(f"net {name} layer {i}: smallest |pre-activation| = {np.abs(pre).min():.3e} of {pre.size}, largest {np.abs(pre).max():.2f}")
            assert pre.size == LARGE[name] and np.abs(pre).max() < 32
            assert np.abs(pre).min() > TIE, "a ReLU pre-activation within 1e-6 of zero: choose SEEDS anew, or for a wide net print NUDGES anew with tools/kinds_nudges.py"
            assert 0.2 < (pre > 0).mean() < 0.8, "the gates must be mixed"


# ---- the mutants ----------------------------------------------------------------------------------------------------------------------------

def _share(got, ref, in_shape, layers, rtol):
    """the worst |d| / allowance of close_per_tensor, without asserting"""
    worst = 0.0
    for ws, bs in tensor_slices(in_shape, layers):
        for t in (ws, bs):
            worst = max(worst, float(np.abs(got[t] - ref[t]).max()) / (rtol * max(1e-3, float(np.abs(ref[t]).max())) + 1e-6))
    return worst


MUTANTS = [("bands16", dict(band_seam=16)), ("bands16", dict(stale_quad=True)), ("bands32", dict(band_seam=32)), ("seam16", dict(band_seam=16)),
           ("seam32", dict(band_seam=32)), ("quads", dict(stale_quad=True)), ("chain", dict(swap_tiles=True))]


@pytest.mark.parametrize("name,mutant", MUTANTS, ids=[f"{n}-{'-'.join(m)}" for n, m in MUTANTS])
def test_the_comparison_of_the_case_sees_its_mutant(name, mutant):
    """On the case's own data each mutant moves the training logits AND the gradient of the gradients call by more than an allowance of
    the loosest run of the case (bf16 where it runs in bf16), the existing mutant tests' factor: the GPU comparison would fail on a
    kernel that made this error.  (A seam at another height than the plan's is no mutant of the case: band_seam = 8 on seam16 differs too,
    but the kernel has no band of 8 rows there.)"""
    in_shape, layers, _ = NETS[name]
    flat, x, y = case(name)
    rtol = max(RTOL[p] for n, p in PAIRS if n == name)
    _, z, g = KindsNet(in_shape, layers, flat).loss_and_grads(x, y)
    _, zm, gm = KindsNet(in_shape, layers, flat, **mutant).loss_and_grads(x, y)
    logits = float(np.abs(zm - z).max()) / (rtol * max(1e-3, float(np.abs(z).max())) + 1e-6)
    share = _share(gm, g, in_shape, layers, rtol)
    print(f"{name} {mutant}: the logits move by {logits:.1f} allowances of rtol {rtol}, the gradient by {share:.1f}")
    assert logits > 1.0 and share > 1.0, (name, mutant, logits, share)


def test_the_mutants_are_what_their_names_say():
    """on a 4 x 2 x 32 map band_seam = 2 changes rows 2 alone, by exactly the taps kh = 0 of row 1; stale_quad changes nothing on a row of
    one slab; swap_tiles exchanges columns 0 .. 31 and 32 .. 63 of a 64-wide 1x1 layer and leaves a 32-wide one alone"""
    from _kinds_cases import BNR, DW, PW
    rng = np.random.default_rng(0)
    layers = ((DW,), BNR, ("dense", 2))
    from _dw_ref import random_params
    flat = random_params(rng, (4, 2, 32), layers)
    x = rng.standard_normal((3, 4, 2, 32))
    outs = {}
    for key, kw in (("ref", {}), ("seam", dict(band_seam=2)), ("stale", dict(stale_quad=True))):
        net = KindsNet((4, 2, 32), layers, flat, **kw)
        net.logits(x, train=False)
        outs[key] = net.outs[0].numpy().transpose(0, 2, 3, 1)
    d = outs["seam"] - outs["ref"]
    w = flat[tensor_slices((4, 2, 32), layers)[0][0]].astype(np.float64).reshape(3, 3, 32)
    lost = np.zeros((3, 2, 32))
    for ww in range(2):
        for kw_ in range(3):
            if 0 <= ww + kw_ - 1 < 2:
                lost[:, ww] += w[0, kw_] * x[:, 1, ww + kw_ - 1]
    assert np.abs(d[:, [0, 1, 3]]).max() == 0 and np.allclose(-d[:, 2], lost, rtol=0, atol=1e-12) and np.abs(lost).max() > 0.1
    assert np.array_equal(outs["stale"], outs["ref"])
    layers = ((PW, 64), BNR, (PW, 32), BNR, ("dense", 2))
    flat = random_params(rng, (1, 2, 32), layers)
    x = rng.standard_normal((2, 1, 2, 32))
    a, b = KindsNet((1, 2, 32), layers, flat), KindsNet((1, 2, 32), layers, flat, swap_tiles=True)
    a.logits(x, train=False), b.logits(x, train=False)
    za, zb = a.outs[0].numpy(), b.outs[0].numpy()
    assert np.array_equal(zb[:, :32], za[:, 32:]) and np.array_equal(zb[:, 32:], za[:, :32]) and not np.array_equal(za, zb)
    layers = ((PW, 32), BNR, ("dense", 2))
    flat = random_params(rng, (1, 2, 32), layers)
    assert np.array_equal(KindsNet((1, 2, 32), layers, flat).logits(x), KindsNet((1, 2, 32), layers, flat, swap_tiles=True).logits(x))


# ---- the exact nets ---------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", sorted(EXACT))
def test_the_integer_nets_are_exact_in_every_precision(name):
    """tests/_dw_ref.py's small-integer net on the wide maps: every operand an integer of at most 8 bits (exact in bf16), |a2| <= 192, every
    logit below H W C 192 + 3 < 2^24 (exact in float32 in any order), and the twin's float64 evaluation gives NumPy's integers"""
    spec = EXACT[name]
    H, W, C = spec[0]
    flat, stats, x, want, a2 = exact_case(spec=spec)
    assert np.abs(x).max() <= 2 and a2.max() <= 192 and H * W * C * 192 + 3 < 2 ** 24 and np.abs(want).max() < 2 ** 24
    for ws, _ in tensor_slices(spec[0], spec[1])[0:5:2]:
        assert set(np.unique(flat[ws])) <= {-1.0, 0.0, 1.0}
    net = DwNet(spec[0], spec[1], flat)
    net.set_bn_stats(stats)
    z = net.logits(x, train=False)
    assert np.array_equal(np.rint(z), want) and np.abs(z - want).max() < 1e-3 * max(1.0, np.abs(want).max())
