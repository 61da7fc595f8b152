"""CPU proof that tests/test_gpu_convnet_bn_forms.py reaches what it claims (cases: tests/_bn_cases.py).  For every FORMS case the plan
(rcn_hipx_plan; options seeded from RCN_HIPX_* as at a net's creation) names the promised kernel forms, the same at every forced grid size,
with at least two items per workgroup in every looping launch of a LOOPING case.  For every SHAPES case the figures of the table -- rows
per partial, partials, row lanes, idle threads, threads per channel, grid.y, streaming workgroups and grid-stride trips -- are worked out
here from (M, C) by csrc/convnet_bn.hpp's rules restated, and held against the plan's text and convnet.bn_partials.  And the reference of
the exact-statistics test proves its teeth: the convolution's output is a float32 value everywhere, the float64 host formula rounds to
what exact rational arithmetic rounds to, and a row left out or counted twice moves every channel by at least 4 float32 ulps.  No GPU
needed, none touched."""
import math
import re
from fractions import Fraction

import numpy as np
import pytest
from _bn_cases import (BF16P_TWIN_LINES, BN_MOMENTUM, FORMS, LOOPING, SHAPES, channel_weights, conv_output, exact_data, host_stats, rows_of,
                       shape_id, shape_spec)
from _torch_ref import TorchNet
from _convnet_util import convnet_built, plan_lines  # noqa: F401  (convnet_built: the fixture `convnet`)
from _forms_cases import SLOTS, env_name, names


def plan_of(convnet, monkeypatch, case, options=None):
    for name, value in (case.options if options is None else options).items():
        monkeypatch.setenv(env_name(name), str(value))
    in_shape, layers, B = case.spec
    return plan_lines(convnet.plan(in_shape, layers, B, precision=case.precision, tiling=case.tiling))


# ---- FORMS -----------------------------------------------------------------------------------------------------------------------------------
def test_case_ids_are_unique_and_every_option_exists():
    from mercer_research_amd import convnet
    assert len({c.id for c in FORMS}) == len(FORMS) and len({shape_id(s) for s in SHAPES}) == len(SHAPES)
    header = open(convnet.HERE + "/csrc/convnet_select.hpp").read()
    for c in FORMS:
        for name in list(c.options) + list(c.twin or {}):
            assert f'{{"{name}", "{env_name(name)}"' in header, name


@pytest.mark.parametrize("case", FORMS, ids=[c.id for c in FORMS])
def test_the_plan_names_the_promised_kernel_forms(convnet, monkeypatch, case):
    L = plan_of(convnet, monkeypatch, case)
    for text in case.lines:
        assert any(names(l, text) for l in L), (text, L)
    # at least one conv_linear layer runs epilogue 1 on an LDS-tiled kernel and does not split K on the implicit GEMM, as every such
    # layer of tests/test_convnet_bn_plan.py's nets behind the first does
    epi1 = [l for l in L if l.startswith("conv3x3") and " epi 1:" in l]
    assert len(epi1) == sum(l[0] == "conv_linear" for l in case.spec[1])
    assert any("k_conv3x3_halo_" in l and "split-K" not in l for l in epi1), epi1


@pytest.mark.parametrize("case", FORMS, ids=[c.id for c in FORMS])
def test_every_looping_launch_has_two_items_per_workgroup_at_every_forced_grid(convnet, monkeypatch, case):
    L = plan_of(convnet, monkeypatch, case)
    items = [(int(m.group(1)), l) for l in L for m in [re.search(r", (\d+) items", l)] if m]
    assert len(items) >= 2, L
    if case in LOOPING:
        for n, l in items:
            assert 2 * max(SLOTS) <= n, l
    # the forced grid is no part of the selection: the plan is the same at every slot count
    for s in SLOTS:
        assert plan_of(convnet, monkeypatch, case, dict(case.options, halo_f32_slots=s)) == L


def test_the_bf16p_twin_differs_in_the_schedule_only(convnet, monkeypatch):
    case = next(c for c in FORMS if c.id == "bn-r128-bf16p")
    a = plan_of(convnet, monkeypatch, case)
    b = plan_of(convnet, monkeypatch, case, case.twin)
    for text in BF16P_TWIN_LINES:
        assert any(names(l, text) for l in b), (text, b)
    strip = lambda l: re.sub(r"k_conv3x3_halo_bf16\w*(<32>)?(, \d+ items)?", "k_conv3x3_halo_bf16*", l)
    assert a != b and [strip(l) for l in a] == [strip(l) for l in b]


# ---- SHAPES: the table's figures from (M, C) ----------------------------------------------------------------------------------------------------
THREADS, FINISH_THREADS, MAX_PARTS, MAX_STREAM = 256, 1024, 512, 4096      # csrc/convnet_bn.hpp


def ceil_div(a, b):
    return -(-a // b)


def rows_per_part(M):
    return max(64, ceil_div(ceil_div(M, MAX_PARTS), 64) * 64)


def team(C):
    s = 1
    while 2 * s * min(C, FINISH_THREADS) <= FINISH_THREADS:
        s *= 2
    return s


def group_blocks(C):
    return ceil_div(C // 4, THREADS)


def stream_blocks(n4, C4):
    q = C4 // math.gcd(C4, THREADS)
    return ceil_div(min(ceil_div(n4, THREADS), MAX_STREAM), q) * q


@pytest.mark.parametrize("s", SHAPES, ids=[shape_id(s) for s in SHAPES])
def test_shape_reaches_what_the_table_says(convnet, s):
    M, C4 = rows_of(s), s.C // 4
    in_shape, layers, B = shape_spec(s)
    assert (("pool",) in layers) == (s.hw[0] % 2 == 0 and s.hw[1] % 2 == 0) and in_shape[2] == 1 and M >= 2 and s.C % 32 == 0
    # rows per partial, partials and the last partial's rows
    R = rows_per_part(M)
    parts = ceil_div(M, R)
    assert (R, parts, M - (parts - 1) * R) == (s.rows, s.parts, s.last)
    assert convnet.bn_partials(M)[0] == parts and convnet.bn_partials(M)[1] >= parts
    # grid.y, and the row lanes and idle threads of the last channel group's workgroups
    gy = group_blocks(s.C)
    cw = C4 - (gy - 1) * THREADS
    assert gy == s.gy and 1 <= cw <= THREADS
    assert (THREADS // cw, THREADS - THREADS // cw * cw) == (s.lanes, s.idle)
    # threads per channel of the finishing workgroup; its rounds; the streaming grid and its trips
    S = team(s.C)
    n4 = M * C4
    blocks = stream_blocks(n4, C4)
    assert (S, blocks, ceil_div(n4, blocks * THREADS)) == (s.team, s.blocks, s.trips)
    assert blocks * THREADS % C4 == 0                      # a thread keeps its four channels along its grid-stride loop
    # ... and the plan says the same
    L = plan_lines(convnet.plan(in_shape, layers, B))
    dims = f"{s.hw[0]}x{s.hw[1]}x{s.C}"
    want = [f"bn-stats {dims}: k_bn_stats, {parts} partials of {R} rows, then k_bn_stats_finish (one workgroup, {S} threads per channel;",
            f"bn-relu {dims}: k_bn_apply_relu, {blocks} workgroups", f"bn-bwd-reduce {dims}: k_bn_bwd_reduce, {parts} partials of {R} rows,",
            f"bn-bwd-dx {dims}: k_bn_bwd_dx, {blocks} workgroups"]
    for text in want:
        assert sum(l.startswith(text) for l in L) == 1, (text, L)


def test_the_table_reaches_every_path_the_statistics_kernels_have():
    """what the notes of the table promise, as arithmetic on its figures (each held against (M, C) above)"""
    by = {shape_id(s): s for s in SHAPES}
    assert rows_of(by["1x2x32-B1"]) == 2
    assert by["1x1x32-B63"].parts == 1 and by["1x1x32-B63"].last < 64 and by["1x1x32-B65"].parts == 2 and by["1x1x32-B65"].last == 1
    assert by["1x1x32-B65"].lanes > by["1x1x32-B65"].last
    for k, lanes in (("1x1x96-B129", 10), ("1x1x160-B129", 6)):
        assert (by[k].lanes, by[k].idle) == (lanes, 16) and by[k].team > by[k].parts
    assert (by["1x1x1024-B66"].lanes, by["1x1x1024-B66"].team) == (1, 1)
    s = by["1x1x1056-B640"]
    assert s.gy == 2 and s.C // 4 - 256 == 8 and s.team == 1 and 8 * s.team < s.parts < 16 * s.team      # two trips of eight partials, the second short
    assert s.C - FINISH_THREADS == 32 and s.blocks % 33 == 0                                             # the second finishing round; the stream grid
    assert by["1x1x1280-B257"].gy == 2 and by["1x1x1280-B257"].C // 4 - 256 == 64
    s = by["16x32x96-B9"]
    assert s.parts == 72 and s.parts % (8 * s.team) != 0 and s.parts > 8 * s.team
    s = by["8x8x32-B513"]
    assert (s.rows, s.parts, s.last) == (128, 257, 64)
    s = by["32x32x128-B33"]
    assert (s.rows, s.parts, s.last, rows_of(s)) == (128, 264, 128, 33792)
    s = by["32x32x32-B130"]
    per_lane = s.rows // s.lanes
    assert (s.rows, s.parts) == (320, 416) and s.rows % s.lanes == 0 and per_lane // 4 == 2 and per_lane % 4 == 2      # two unrolled trips, a tail of two
    assert s.blocks == MAX_STREAM and s.trips == 2
    s = by["32x32x96-B43"]
    assert s.blocks == 4098 and s.blocks % 3 == 0 and s.trips == 2
    # more than 64 rows per partial, which no other BN test runs
    assert sum(s.rows > 64 for s in SHAPES) >= 4


# ---- SHAPES: the exact reference proves its teeth ------------------------------------------------------------------------------------------------
def ulps32(a, b):
    """|a - b| in units of the float32 spacing at b, elementwise (float64 in)"""
    return np.abs(a - b) / np.spacing(np.abs(b).astype(np.float32)).astype(np.float64)


@pytest.mark.parametrize("s", SHAPES, ids=[shape_id(s) for s in SHAPES])
def test_the_exact_reference_has_teeth(s):
    flat, v, _ = exact_data(s)
    in_shape, layers, B = shape_spec(s)
    M, C = rows_of(s), s.C
    x = conv_output(s, v)
    # (i) the convolution's output is a float32 value everywhere, positive, channels distinct -- and IS what the float64 twin's own
    # convolution makes of the parameters the device gets (the layout of the taps, not only the formula)
    assert np.abs(v).max() <= 8 and np.array_equal(v, np.round(v))
    assert np.array_equal(x, x.astype(np.float32).astype(np.float64)) and x.min() >= 8.0
    assert len(set(zip(*channel_weights(C)))) == C
    import torch
    with torch.no_grad():
        conv = TorchNet(in_shape, layers, flat).mods[0]
        xt = conv(torch.from_numpy(v.astype(np.float64).transpose(0, 3, 1, 2))).permute(0, 2, 3, 1).reshape(M, C).numpy()
    assert np.array_equal(xt, x)
    # (ii) the float64 host formula, rounded to float32, is the rounding of the exact rational value: |r - f| <= half a spacing of f
    host = host_stats(x)
    f32 = host.astype(np.float32)
    X = np.round(x * 8).astype(np.int64)                   # x in eighths: exact integers
    assert np.array_equal(X / 8.0, x)
    s1, s2 = [int(t) for t in X.sum(axis=0)], [int(t) for t in (X * X).sum(axis=0)]
    mom = Fraction(BN_MOMENTUM)
    for c in range(C):
        mean = Fraction(s1[c], 8 * M)
        var = Fraction(s2[c], 64 * M) - mean * mean
        assert var >= 0
        for got, r in ((f32[c], mom * mean), (f32[C + c], (1 - mom) + mom * var * M / (M - 1))):
            assert 2 * abs(r - Fraction(float(got))) <= Fraction(float(np.spacing(got))), (c, got, float(r))
    # (iii) a row left out of the sums, or counted twice, with M unchanged, moves the mean or the variance of EVERY channel by >= 4 ulps
    for name, xm in (("the last row left out", x[:-1]), ("the first row twice", np.concatenate([x[:1], x]))):
        d = ulps32(host_stats(xm, M=M), host)
        moved = np.maximum(d[:C], d[C:])
        print(f"{shape_id(s)} {name}: the least-moved channel moves by {moved.min():.0f} ulps")
        assert moved.min() >= 4.0, (name, int(moved.argmin()), float(moved.min()))
    # ... so does exchanging two channels' biases (the channels are distinct)
    w, b = channel_weights(C)
    b[[0, C - 1]] = b[[C - 1, 0]]
    d = ulps32(host_stats(v.astype(np.float64).reshape(-1, 1) * w + b), host)
    assert d[0] >= 4.0 and d[C - 1] >= 4.0
