"""The cases of tests/test_gpu_convnet_bn_forms.py (GPU, against float64 torch: tests/_torch_ref.py) and tests/test_convnet_bn_forms_plan.py
(CPU: the proof, by rcn_hipx_plan, that every case reaches what it names, and that the exact-statistics reference has teeth).  ONE table,
so that the two files cannot drift apart; Case, names, env_name and SLOTS are tests/_forms_cases.py's.  Not a test file and not a conftest.

Two groups:
  FORMS    batch-normalised nets at the sizes where the second conv_linear layer no longer splits K on the implicit-GEMM kernels: epilogue 1
           (bias only) of the LDS-tiled convolution kernels, their epilogue-3 input gradients gated by a BN layer's output, and the looping
           forms with several items per workgroup (LOOPING: every "items" line has at least 2 * max(SLOTS) items).
  SHAPES   one conv_linear -> bn_relu layer on a single-channel input at the (M, C) where the statistics kernels take another path.  Their
           data (`exact_data`) makes the convolution's output exact, so the running statistics can be held to one float32 ulp."""
from collections import namedtuple

import numpy as np
from _torch_ref import random_params, tensor_slices
from _forms_cases import Case

CL, BN, POOL = "conv_linear", ("bn_relu",), ("pool",)

# ---- FORMS -----------------------------------------------------------------------------------------------------------------------------------
# tests/_forms_cases.py's WIDE16 and PAIRS8 with a BN layer behind every convolution but one: 8 x 16 blocks of one image, three column
# blocks, the pooled map's layers; 8 x 8 blocks of two images with an odd batch, and a ReLU convolution above a BN layer (pooled-in epi 3)
BN_WIDE16 = ((16, 32, 3), ((CL, 32), BN, (CL, 96), BN, POOL, (CL, 96), BN, POOL, ("dense", 10)), 5)
BN_PAIRS8 = ((24, 24, 1), ((CL, 32), BN, (CL, 64), BN, POOL, (CL, 64), BN, ("conv", 64), POOL, ("dense", 7)), 7)
# 33792 rows: 264 partials of 128 rows, and 264 output tiles of 32 -> 32 (no split-K)
BN_R128 = ((32, 32, 3), ((CL, 32), BN, (CL, 32), BN, POOL, ("dense", 10)), 33)
# tests/_forms_cases.py's BF16_HALO_PLAIN with BN: 264 tiles in 32 -> 96 and in the input gradient of 96 -> 64, which a BN layer's output gates
BN_PLAIN96 = ((16, 32, 3), ((CL, 32), BN, (CL, 96), BN, (CL, 64), BN, POOL, ("dense", 10)), 22)

_R128_STATS = "bn-stats 32x32x32: k_bn_stats, 264 partials of 128 rows"
FORMS = [
    Case("bn-wide16-lds", BN_WIDE16, "fp32", "lds", {},
         ["16x32x32->96 epi 1: k_conv3x3_halo_f32<16, 32>, 60 items", "8x16x96->96 epi 1: k_conv3x3_halo_f32<16, 32>, 15 items",
          "8x16x96->96 epi 0: k_conv3x3_halo_f32<16, 32>, 15 items", "16x32x96->32 epi 3: k_conv3x3_halo_f32<16, 32>, 20 items"]),
    Case("bn-pairs8-lds", BN_PAIRS8, "fp32", "lds", {},
         ["24x24x32->64 epi 1: k_conv3x3_halo_f32<8, 64>, 36 items", "12x12x64->64 epi 1: k_conv3x3_halo_f32<16, 64>, 14 items",
          "12x12x64->64 epi 3 pooled-in: k_conv3x3_halo_f32<16, 64>, 14 items", "24x24x64->32 epi 3: k_conv3x3_halo_f32<8, 32>, 36 items"]),
    Case("bn-r128-fp32", BN_R128, "fp32", "auto", {},
         [_R128_STATS, "32x32x32->32 epi 1: k_conv3x3_halo_f32<16, 32>, 264 items", "32x32x32->32 epi 3: k_conv3x3_halo_f32<16, 32>, 264 items"]),
    Case("bn-r128-1cb", BN_R128, "bf16", "auto", {},
         [_R128_STATS, "32x32x32->32 epi 1: k_conv3x3_halo_bf16_1cb<32>, 264 items", "32x32x32->32 epi 3: k_conv3x3_halo_bf16_1cb<32>, 264 items"]),
    Case("bn-r128-bf16p", BN_R128, "bf16", "auto", {"bf16_1cb": 0},
         [_R128_STATS, "32x32x32->32 epi 1: k_conv3x3_halo_bf16p, 264 items", "32x32x32->32 epi 3: k_conv3x3_halo_bf16p, 264 items"],
         {"bf16_1cb": 0, "bf16_pipe": 0}),
    Case("bn-plain96-bf16", BN_PLAIN96, "bf16", "auto", {},
         ["16x32x32->96 epi 1: k_conv3x3_halo_bf16_1cb<32>, 264 items", "16x32x64->96 epi 3: k_conv3x3_halo_bf16p, 264 items", "bn-stats 16x32x96"]),
]
# what the twin of bn-r128-bf16p must name instead (one workgroup per item: its lines carry no item count)
BF16P_TWIN_LINES = ["32x32x32->32 epi 1: k_conv3x3_halo_bf16", "32x32x32->32 epi 3: k_conv3x3_halo_bf16"]
# the cases run on forced grids of SLOTS workgroups
LOOPING = [c for c in FORMS if c.id in ("bn-wide16-lds", "bn-pairs8-lds", "bn-r128-1cb", "bn-r128-bf16p")]


def conv_linear_layers(layers):
    """the indices, among the layers with parameters, of the bias-only convolutions in front of a BN layer: their bias GRADIENT is zero in
    exact arithmetic (close_per_tensor's bias_at_weight_scale)"""
    return tuple(i for i, l in enumerate(l for l in layers if l[0] != "pool") if l[0] == CL)


# ---- SHAPES ----------------------------------------------------------------------------------------------------------------------------------
# (H, W), C, B and what the statistics kernels do there (csrc/convnet_bn.hpp), each figure asserted by tests/test_convnet_bn_forms_plan.py:
#   rows      rows per partial (bn_rows_per_part)          parts     partials (grid.x of k_bn_stats / k_bn_bwd_reduce)
#   last      rows of the last partial                     lanes     row lanes of the LAST channel group's workgroups (256 / channel groups)
#   idle      its threads past lanes * channel groups      team      threads per channel of the finishing workgroup (bn_team)
#   gy        grid.y: workgroups of 256 channel groups     blocks    workgroups of k_bn_apply_relu / k_bn_bwd_dx (bn_stream_blocks)
#   trips     the most grid-stride trips of a thread of those two kernels
Shape = namedtuple("Shape", "hw C B rows parts last lanes idle team gy blocks trips note")
SHAPES = [
    Shape((1, 2), 32, 1, 64, 1, 2, 32, 0, 32, 1, 1, 1, "the smallest legal M"),
    Shape((1, 1), 32, 63, 64, 1, 63, 32, 0, 32, 1, 2, 1, "one clipped partial; lanes past the rows' end in the tail"),
    Shape((1, 1), 32, 65, 64, 2, 1, 32, 0, 32, 1, 3, 1, "a second partial of one row: 31 row lanes without a row"),
    Shape((1, 1), 96, 129, 64, 3, 1, 10, 16, 8, 1, 15, 1, "10 row lanes and 16 idle threads; a team of 8 > 3 partials"),
    Shape((1, 1), 160, 129, 64, 3, 1, 6, 16, 4, 1, 25, 1, "6 row lanes and 16 idle threads; a team of 4 > 3 partials"),
    Shape((1, 1), 1024, 66, 64, 2, 2, 1, 0, 1, 1, 66, 1, "C / 4 = 256: one row lane, a team of 1"),
    Shape((1, 1), 1056, 640, 64, 10, 64, 32, 0, 1, 2, 660, 1, "grid.y = 2 with a last group of 8; 10 partials in trips of 8; a second finishing round of 32 threads; 660 = 33 * 20"),
    Shape((1, 1), 1280, 257, 64, 5, 1, 4, 0, 1, 2, 325, 1, "a last channel group of 64"),
    Shape((16, 32), 96, 9, 64, 72, 64, 10, 16, 8, 1, 432, 1, "72 partials against 8 * S = 64"),
    Shape((8, 8), 32, 513, 128, 257, 64, 32, 0, 32, 1, 1026, 1, "257 partials of 128 rows, the last of 64"),
    Shape((32, 32), 128, 33, 128, 264, 128, 8, 0, 8, 1, 4096, 2, "264 x 128 rows at the workload's widest layer"),
    Shape((32, 32), 32, 130, 320, 416, 320, 32, 0, 32, 1, 4096, 2, "416 partials of 320 rows: ten rows per lane, two unrolled trips and a tail of two; a second grid-stride trip"),
    Shape((32, 32), 96, 43, 128, 344, 128, 10, 16, 8, 1, 4098, 2, "4098 workgroups (a multiple of 3) and a second trip"),
]
BN_MOMENTUM, BN_EPS = 0.5, 1e-5                         # set_bn of the exact test: from reset statistics, 0.5 exposes the batch's own


def shape_id(s):
    return f"{s.hw[0]}x{s.hw[1]}x{s.C}-B{s.B}"


def shape_spec(s):
    H, W = s.hw
    pool = (POOL,) if H % 2 == 0 and W % 2 == 0 else ()
    return ((H, W, 1), ((CL, s.C), BN) + pool + (("dense", 4),), s.B)


def rows_of(s):
    return s.B * s.hw[0] * s.hw[1]


def channel_weights(C):
    """(w_c, b_c) of the exact construction: x[m, c] = w_c * v[m] + b_c with v integer in [-8, 8] is a multiple of 1/8 in [8, 32 + C/8 + 24]
    -- positive, a float32 value, and no two channels share (w_c, b_c)"""
    c = np.arange(C)
    return (1 + c % 3).astype(np.float64), 32.0 + c / 8.0


def exact_data(s):
    """(flat parameters, v[B][H][W][1], labels) of a SHAPES case: integer inputs, a convolution of the centre tap alone, gamma, beta and
    the dense layer random.  Deterministic per case; float32 / int32, as the device takes them."""
    in_shape, layers, B = shape_spec(s)
    rng = np.random.default_rng(1000 * s.C + rows_of(s))
    flat = random_params(rng, in_shape, layers)
    (ws, bs) = tensor_slices(in_shape, layers)[0]
    w, b = channel_weights(s.C)
    taps = np.zeros((9, s.C))
    taps[4] = w                                          # K = 9 * Cin rows of [ky][kx][cin]: the centre tap is row 4
    flat[ws], flat[bs] = taps.ravel(), b
    v = rng.integers(-8, 9, (B,) + in_shape).astype(np.float32)
    y = rng.integers(0, 4, B).astype(np.int32)
    return flat, v, y


def conv_output(s, v):
    """x[M][C] in float64: what the convolution of exact_data's parameters makes of v -- every product and sum exact"""
    w, b = channel_weights(s.C)
    return v.astype(np.float64).reshape(-1, 1) * w + b


def host_stats(x, M=None, momentum=BN_MOMENTUM):
    """ConvNet.get_bn_stats's [running mean | running var] after ONE training forward from reset statistics (0, 1) over the rows of x, in
    float64 by csrc/convnet_bn.hpp's formula: mean = s / M, var = q / M - mean^2 (biased), running var from var * M / (M - 1).  The sums
    s and q are exact in float64 on exact_data's x (multiples of 1/8 and 1/64 far below 2^53).  M: the divisor, where it is not the
    number of rows of x (the mutants of the teeth test)."""
    M = x.shape[0] if M is None else M
    s, q = x.sum(axis=0), (x * x).sum(axis=0)
    mean = s / M
    var = np.maximum(0.0, q / M - mean * mean)
    return np.concatenate([(1.0 - momentum) * 0.0 + momentum * mean, (1.0 - momentum) * 1.0 + momentum * (var * M / (M - 1))])
