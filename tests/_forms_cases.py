"""The cases of tests/test_gpu_convnet_forms.py (GPU, against the oracle) and tests/test_convnet_forms_plan.py (CPU: the proof, by
rcn_hipx_plan, that every case reaches the kernel forms it names).  ONE table, so that the two files cannot drift apart.  Not a test file
and not a conftest.

A case is (id, net spec = (in_shape, layers, B), precision, tiling, options, lines): `options` are rcn_hipx_set_option names and values,
`lines` are texts each of which some line of the case's plan must contain.  Three groups:
  LOOPS    the looping kernels (launch_resident) with the grid forced down to SLOTS workgroups by "halo_f32_slots": every looping launch
           of the case's plan has at least 2 * max(SLOTS) items, so every workgroup takes a second item at every slot count;
  WGRADS   more than one pixel block per chunk of the LDS-tiled weight gradients (the chunk counts in `lines` are below the layers'
           pixel-block counts, and at least one chunk of every case is shorter than the others);
  OPTIONS  kernel forms that only an option selects.  `twin`: option values under which the same arithmetic runs in another schedule --
           results are compared bit for bit with the case's own."""
import re
from collections import namedtuple

Case = namedtuple("Case", "id spec precision tiling options lines twin", defaults=(None,))

SLOTS = (1, 2, 3, 5, 7)                                   # forced grid sizes of the looping kernels ("halo_f32_slots")

# ---- nets ----------------------------------------------------------------------------------------------------------------------------------
# 8 x 16 blocks of one image; 32 -> 96: three column blocks x two block columns x two block rows (every carry of advance());
# 96 -> 96 on the pooled map: three channel blocks; their input gradients read pooled-resolution gradients (EPI 3 and EPI 0)
WIDE16 = ((16, 32, 3), (("conv", 32), ("conv", 96), ("pool",), ("conv", 96), ("pool",), ("dense", 10)), 5)
# 8 x 8 blocks of two images with an odd batch (24-wide maps), 8 x 16 blocks on the 12 x 12 map; two channel blocks in 64 -> 64 and 64 -> 32
PAIRS8 = ((24, 24, 1), (("conv", 32), ("conv", 64), ("pool",), ("conv", 64), ("pool",), ("dense", 7)), 7)
# bf16 storage: 32 -> 32 with the fused pool (resident weights or pipelined), 32 -> 64, 64 -> 64 with the fused pool; input gradients with
# and without a pooled-resolution input
STORED = ((24, 32, 1), (("conv", 32), ("conv", 32), ("pool",), ("conv", 64), ("conv", 64), ("pool",), ("dense_relu", 64), ("dense", 10)), 7)
STORED_ITEMS = ["24x32x1->32 epi 2: k_conv1_fwd_f32<1, 16>", "epi 2: k_conv3x3_halo_bf16p,", "12x16x64->64 epi 4: k_conv3x3_halo_bf16p,",
                "12x16x64->64 epi 3 pooled-in: k_conv3x3_halo_bf16p,", "12x16x64->32 epi 0: k_conv3x3_halo_bf16p,"]
# (also a net of OPTIONS, below)
# 264 output tiles in 32 -> 96 and in the input gradient of 96 -> 64 (64 -> 96): no split-K, so the bf16 LDS-tiled kernels with epilogues 2 and 3
BF16_HALO_PLAIN = ((16, 32, 3), (("conv", 32), ("conv", 96), ("conv", 64), ("pool",), ("dense", 10)), 22)

LOOPS = [
    Case("fp32-16wide", WIDE16, "fp32", "lds", {},
         ["epi 2: k_conv1_fwd_f32<3, 16>, 20 items", "16x32x32->96 epi 4: k_conv3x3_halo_f32<16, 32>, 60 items", "8x16x96->96 epi 4: k_conv3x3_halo_f32<16, 32>, 15 items",
          "8x16x96->96 epi 0 pooled-in: k_conv3x3_halo_f32<16, 32>, 15 items", "16x32x96->32 epi 3 pooled-in: k_conv3x3_halo_f32<16, 32>, 20 items"]),
    Case("fp32-8wide-pairs", PAIRS8, "fp32", "lds", {},
         ["epi 2: k_conv1_fwd_f32<1, 8>, 36 items", "24x24x32->64 epi 4: k_conv3x3_halo_f32<8, 64>, 36 items", "12x12x64->64 epi 4: k_conv3x3_halo_f32<16, 64>, 14 items",
          "12x12x64->64 epi 0 pooled-in: k_conv3x3_halo_f32<16, 64>, 14 items", "24x24x64->32 epi 3 pooled-in: k_conv3x3_halo_f32<8, 32>, 36 items"]),
    # 32 -> 96 with the fused pool: the resident-weights kernel with three column blocks -- at 1 and 2 workgroups a workgroup changes column
    # block between items (the reload of its weights and bias registers), at 3 never
    Case("bf16-1cb-reload", WIDE16, "bf16", "auto", {},
         ["epi 2: k_conv1_fwd_f32<3, 16>, 20 items", "16x32x32->96 epi 4: k_conv3x3_halo_bf16_1cb<32>, 60 items"]),
    Case("stored-1cb", STORED, "bf16_stored", "auto", {"bf16_1cb": 1},
         STORED_ITEMS + ["24x32x32->32 epi 4: k_conv3x3_halo_bf16_1cb<32>,", "24x32x32->32 epi 3 pooled-in: k_conv3x3_halo_bf16_1cb<32>,"]),
    Case("stored-pipelined", STORED, "bf16_stored", "auto", {"bf16_1cb": 0},
         STORED_ITEMS + ["24x32x32->32 epi 4: k_conv3x3_halo_bf16p,", "24x32x32->32 epi 3 pooled-in: k_conv3x3_halo_bf16p,"]),
    # the pipelined kernel with THREE column blocks (the stored cases have one: the carry out of the column-block digit never runs there)
    Case("bf16-pipelined-3-column-blocks", BF16_HALO_PLAIN, "bf16", "auto", {},
         ["epi 2: k_conv1_fwd_f32<3, 16>, 88 items", "16x32x32->96 epi 2: k_conv3x3_halo_bf16_1cb<32>, 264 items", "16x32x64->96 epi 3: k_conv3x3_halo_bf16p, 264 items"]),
]

# ---- weight-gradient chunks of several pixel blocks --------------------------------------------------------------------------------------------
# full-resolution dZ (32 -> 32, a convolution behind it) and pooled dZ (the layer in front of the pool), 20 pixel blocks each
WG16 = ((16, 32, 3), (("conv", 32), ("conv", 32), ("conv", 96), ("pool",), ("dense", 10)), 5)
# the same on 8 x 8 blocks of two images: 27 pixel blocks
WG8 = ((24, 24, 1), (("conv", 32), ("conv", 32), ("conv", 64), ("pool",), ("dense", 7)), 5)
# the first layer's kernel aims at 1024 workgroups: 8 tiles x 129 pixel blocks -> 65 chunks of 2, the last of 1
WG_FIRST = ((24, 16, 3), (("conv", 256), ("pool",), ("dense", 10)), 43)
# bf16 storage: 20 pixel blocks in chunks of 8, 8 and 4
WG_STORED = ((16, 32, 1), STORED[1], 5)

WGRADS = [
    Case("wg16-one-chunk", WG16, "fp32", "lds", {"wgh_f32_target": 1},
         ["16x32x32->32: k_wgrad3x3_halo_f32<16>, 1 chunks x 1 tiles", "16x32x32->96 pooled-dZ: k_wgrad3x3_halo_f32<16>, 1 chunks x 3 tiles"]),
    Case("wg16-ragged", WG16, "fp32", "lds", {"wgh_f32_target": 9},
         ["16x32x32->32: k_wgrad3x3_halo_f32<16>, 7 chunks x 1 tiles", "16x32x32->96 pooled-dZ: k_wgrad3x3_halo_f32<16>, 3 chunks x 3 tiles"]),
    Case("wg8-one-chunk", WG8, "fp32", "lds", {"wgh_f32_target": 1},
         ["24x24x32->32: k_wgrad3x3_halo_f32<8>, 1 chunks x 1 tiles", "24x24x32->64 pooled-dZ: k_wgrad3x3_halo_f32<8>, 1 chunks x 2 tiles"]),
    Case("wg8-ragged", WG8, "fp32", "lds", {"wgh_f32_target": 8},
         ["24x24x32->32: k_wgrad3x3_halo_f32<8>, 7 chunks x 1 tiles", "24x24x32->64 pooled-dZ: k_wgrad3x3_halo_f32<8>, 4 chunks x 2 tiles"]),
    Case("wg-first-layer", WG_FIRST, "fp32", "lds", {},
         ["24x16x3->256 pooled-dZ: k_conv1_wgrad_f32<3, 16>, 65 chunks"]),
    Case("wg-stored-ragged", WG_STORED, "bf16_stored", "auto", {},
         ["16x32x32->32 pooled-dZ: k_wgrad3x3_halo_bf16<32, 32>, 3 chunks x 1 tiles"]),
]

# ---- forms only an option selects ---------------------------------------------------------------------------------------------------------------
# a 4 x 8 map: B * 32 pixels per convolution, in chunks of 128 ("pix_per_chunk"): 1, 5 and 9 chunks -- under "xcd_remap" 7, 3 and 7 padding
# workgroups per tile that return early, and at 9 chunks a second group of eight
def _flat48(B):
    return ((4, 8, 3), (("conv", 32), ("conv", 64), ("dense_relu", 32), ("dense", 10)), B)


# 64-multiple widths: the 64-wide column blocks of the implicit-GEMM weight gradients, which the policies narrow at this size
WIDTHS64 = ((8, 8, 3), (("conv", 64), ("conv", 64), ("pool",), ("dense_relu", 64), ("dense", 10)), 4)
# dense weight gradients of 4, 2 and 1 k-blocks per workgroup, by shape.  40 classes: no fused head whatever "head" says ("head" = 0 on a
# fusable head would round the logits layer's operands, which the oracle -- head_is_fp32, by shape -- does not mirror)
DENSE_NK = ((4, 4, 3), (("conv", 32), ("pool",), ("dense_relu", 64), ("dense_relu", 32), ("dense", 40)), 4)
# a 32-channel and a 64-channel layer on the bf16 LDS-tiled kernels with the pool fused (at this size the layers without a pool split K on
# the implicit-GEMM kernel)
BF16_HALO = ((16, 16, 3), (("conv", 32), ("conv", 64), ("pool",), ("conv", 64), ("conv", 32), ("pool",), ("dense", 10)), 4)

_REMAP = {"xcd_remap": 1, "pix_per_chunk": 128}
OPTIONS = [
    Case(f"xcd-remap-fp32-{c}chunks", _flat48(B), "fp32", "gemm", _REMAP,
         [f"4x8x3->32: k_conv_wgrad<3, gather, 32>, {c} chunks", f"4x8x32->64: k_conv_wgrad<3, tile, 32>, {c} chunks"], {"xcd_remap": 0})
    for B, c in ((4, 1), (20, 5), (36, 9))
] + [
    Case(f"xcd-remap-bf16-{c}chunks", _flat48(B), "bf16", "auto", dict(_REMAP, halo_wgrad=0),
         [f"4x8x3->32: k_conv_wgrad<3, gather, 32>, {c} chunks", f"4x8x32->64: k_conv_wgrad_bf16<3, 32, 3>, {c} chunks"], dict(_REMAP, halo_wgrad=0, xcd_remap=0))
    for B, c in ((4, 1), (20, 5), (36, 9))
] + [
    # select_conv: "same LDS images, rounding and MFMA order" as the pipelined forms -- hence the twin
    Case("bf16-not-pipelined", BF16_HALO, "bf16", "auto", {"bf16_pipe": 0},
         ["16x16x32->64 epi 4: k_conv3x3_halo_bf16", "8x8x64->32 epi 4: k_conv3x3_halo_bf16"], {"bf16_pipe": 1}),
    Case("bf16-not-pipelined-plain", BF16_HALO_PLAIN, "bf16", "auto", {"bf16_pipe": 0},
         ["16x32x32->96 epi 2: k_conv3x3_halo_bf16", "16x32x64->96 epi 3: k_conv3x3_halo_bf16"], {"bf16_pipe": 1}),
    Case("bf16-no-lds-tiling", BF16_HALO, "bf16", "auto", {"halo": 0},
         ["16x16x32->64 epi 2: k_conv_fwd_bf16<3, tile,", "8x8x64->32 epi 2: k_conv_fwd_bf16<3, tile,", "k_pool_fwd", "k_pool_bwd"]),
    Case("fp32-implicit-gemm-wgrad", WIDE16, "fp32", "lds", {"halo_wgrad": 0},
         ["16x32x32->96 epi 4: k_conv3x3_halo_f32<16, 32>", "epi 3: k_conv3x3_halo_f32<16, 32>", "k_pool_bwd", "16x32x3->32: k_conv_wgrad<3, gather, 32>",
          "16x32x32->96: k_conv_wgrad<3, tile, 32>", "8x16x96->96: k_conv_wgrad<3, tile, 32>"]),
    Case("bf16-implicit-gemm-wgrad", BF16_HALO, "bf16", "auto", {"halo_wgrad": 0},
         ["16x16x32->64: k_conv_wgrad_bf16<3, 32, 3>", "8x8x64->32: k_conv_wgrad_bf16<3, 32, 3>", "k_pool_bwd"]),
    Case("fp32-unfused-pool-bwd", WIDE16, "fp32", "lds", {"fuse_pool_bwd": 0},
         ["k_pool_bwd", "8x16x96->96 epi 0: k_conv3x3_halo_f32<16, 32>", "16x32x96->32 epi 3: k_conv3x3_halo_f32<16, 32>", "16x32x32->96: k_wgrad3x3_halo_f32<16>",
          "8x16x96->96: k_wgrad3x3_halo_f32<16>"]),
    Case("fp32-64wide-wgrad", WIDTHS64, "fp32", "gemm", {"wgf_policy": 0},
         ["8x8x64->64: k_conv_wgrad<3, tile, 64>", "1x1x1024->64: k_conv_wgrad<1, tile, 64>"]),
    Case("bf16-64wide-wgrad", WIDTHS64, "bf16", "auto", {"wgb_policy": 0, "halo_wgrad": 0},
         ["8x8x64->64: k_conv_wgrad_bf16<3, 64, 3>", "1x1x1024->64: k_conv_wgrad_bf16<1, 64, 4>"]),
    Case("bf16-dense-nk", DENSE_NK, "bf16", "auto", {"head": 0},
         ["1x1x128->64: k_conv_wgrad_bf16<1, 32, 4>", "1x1x64->32: k_conv_wgrad_bf16<1, 32, 2>", "1x1x32->64: k_conv_wgrad_bf16<1, 32, 1>", "k_softmax_ce"]),
]

CASES = LOOPS + WGRADS + OPTIONS


def names(line, text):
    """`text` stands in `line` as whole words: k_conv3x3_halo_bf16 is not found in k_conv3x3_halo_bf16p, nor 1 chunks in 11 chunks"""
    return re.search(f"(?<![A-Za-z0-9_]){re.escape(text)}(?![A-Za-z0-9_])", line) is not None


def env_name(option):
    """the environment variable that seeds `option` where a plan or a net is created (csrc/convnet_select.hpp, kXOptTable)"""
    return "RCN_HIPX_" + option.upper()
