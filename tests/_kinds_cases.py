"""The one table of cases of tests/test_convnet_kinds_forms_plan.py (CPU) and tests/test_gpu_convnet_kinds_forms.py (GPU): the forms of the
stride-2, 1x1 and depthwise kernels (csrc/convnet_dw.hpp, csrc/convnet_pw.hpp, csrc/convnet_select.hpp) that the nets of the three kind
files leave unlaunched.  Per case the input shape, layers and batch (NETS), the device runs with their precision and options (RUNS), the
seeds (SEEDS) and what the plan must say it reaches (DW_TILES, PW_NT, ...); the CPU file proves the last from the plan text, and the
premises of the comparison from the twin alone.  The reference is tests/_dw_ref.py's DwNet (all twelve kinds) on tests/_twin_checks.py's
schedule at the stride file's bounds; nothing of either is copied here.  `KindsNet` adds three MUTANTS to DwNet, never a model of the library.

The ReLU gates of the large maps.  A band of 16 or 32 rows is planned only at 1024 tiles or more, so the nets that plan one have 1 to 18
million elements per ReLU map.  The device decides a gate on a float32 pre-activation that is a few 1e-7 off the twin's float64 one, and
an element gated the other way moves a weight gradient by one whole term of its sum (tests/_stride_ref.py records seven fp32 allowances
for one such element).  tests/_stride_ref.py's rule is that no pre-activation lies within 1e-6 of zero.  With a density of 0.4 at zero
a map of n elements is expected to hold 0.8e-6 n of them (4 to 14 per map of the wide nets were counted), so for the wide nets seeds
alone do not give it: a depthwise net keeps its channels apart, and NUDGES moves the beta of each channel that holds such an element by
a multiple of 1e-5, found from the twin alone; the CPU file asserts the rule on the parameters as `case` returns them.
Not a test file and not a conftest: every assert carries its message."""
import numpy as np
from _dw_ref import DW, PW, X_SPEC, DwNet, random_params, tensor_slices

BNR = ("bn_relu",)
HEAD = (("global_avgpool",), ("dense", 10))
DW2 = ((DW,), BNR, (DW,), BNR) + HEAD            # a depthwise layer as layer 0 (forward only) and one with a gated input gradient


def chain(*widths):
    """1x1 layers of these widths, a bn_relu behind each, then the head"""
    out = ()
    for c in widths:
        out += ((PW, c), BNR)
    return out + HEAD


STEM = (8, 12, 3)
SEPDOWN = (("conv_linear", 32), BNR, (DW,), BNR, ("conv_linear_s2", 64), ("bn_add_relu_down", 4))

# (input shape, layers, batch)
NETS = {
    # ---- k_dw: band heights 16 and 32 (select_dw takes them at 1024 tiles or more), two slabs per row, 46080 to 71680 pixels in the weight gradient
    # th = 16, two bands of 16 + 4 rows x two slabs of 256 + 8 pieces, 24 quads: the seam's halo rows come from the neighbouring band, the last
    # band is partial, a lane's quad differs between the slabs by 256 % 24 = 16 (on three looping workgroups it changes on every tile);
    # forward as layer 0, forward and gated input gradient; the weight gradient in 440 chunks of 128 pixels
    "bands16": ((20, 11, 96), DW2, 256),
    # th = 32 on H = 28: ONE band taller than the map x two slabs, the whole-height form of the kernel's header and of cifar_sep; the weight
    # gradient by the default chunk formula above its 128-pixel floor (280 chunks of 256 pixels)
    "band32": ((28, 5, 256), DW2, 512),
    # th = 32, two bands of 32 + 4 rows x two slabs
    "bands32": ((36, 5, 256), DW2, 256),
    # ---- the same band forms on the narrowest maps that plan them (one slab per row), where seeds alone meet the rule on the ReLU gates
    # th = 16, two bands of 16 + 4 rows: the halo rows h0 - 1 and h0 + 16 come from the neighbouring band, the last band is partial
    "seam16": ((20, 3, 32), DW2, 512),
    # th = 32 on H = 28: ONE band taller than the map, the whole-height form of the kernel's header; with wg_target = 256 its weight
    # gradient takes the default chunk formula above the 128-pixel floor (224 chunks of 256 pixels)
    "whole32": ((28, 2, 32), DW2, 1024),
    # th = 32, two bands of 32 + 4 rows
    "seam32": ((36, 2, 32), DW2, 512),
    # C / 4 = 24 quads and 264 pieces per row = two slabs (8 live lanes in the second): a lane's quad differs between the slabs by 256 % 24 = 16.
    # On three looping workgroups a workgroup's consecutive tiles alternate between the slabs, so the weights are reloaded on every tile
    "quads": ((10, 11, 96), DW2, 2),
    # ---- k_pw: every NT in 1 .. 8, K-tile counts 1, 2, 3, 5, 6, 7; M = 175: one full and one partial row block
    "chain": ((5, 7, 32), chain(192, 64, 224, 64, 160, 96, 32), 5),
    # the slice limit in fp32: [512][32] is exactly 80 KB of dynamic LDS; 544 is the first contraction no 32-wide slice holds
    "limit32": ((4, 4, 32), chain(512, 64, 544, 32), 3),
    # ... and with bf16 operands: [1024][32], 1056
    "limit16": ((4, 4, 32), chain(1024, 64, 1056, 32), 3),
    # ---- the kinds composed with each other's skip kernels
    # the downsampling bottleneck (option-A shortcut): a 1x1 layer above the skip's source, k_skip_bwd_add_down behind its input gradient
    "neck": (STEM, (("conv_linear", 64), BNR, (PW, 32), BNR, ("conv_linear_s2", 32), BNR, (PW, 128), ("bn_add_relu_down", 6)) + HEAD, 4),
    # the separable downsampling block: k_dw<3> directly in front of k_skip_bwd_add_down
    "sepdown": (STEM, SEPDOWN + HEAD, 4),
    # ... continued by a residual separable block: a depthwise layer on a strided layer's map, both skip kernels in one net
    "sepdown2": (STEM, SEPDOWN + ((DW,), BNR, (PW, 64), ("bn_add_relu", 4)) + HEAD, 4),
    # ---- the smallest maps
    # 2 x 2 -> 1 x 1: every parity class of the strided input gradient sees exactly one output pixel
    "s2x2": ((4, 4, 3), (("conv", 32), ("pool",), ("conv_linear_s2", 64), BNR, ("conv_linear", 64), ("bn_add_relu_down", 4), ("dense", 4)), 2),
    # a 1 x 1 map: all eight outer taps of k_dw meet a border; above a pool (epilogue 0)
    "dw1x1": ((2, 2, 3), (("conv", 32), ("pool",), (DW,), BNR, (PW, 32), BNR, ("dense", 4)), 2),
    # H = 1: the rows above and below are never inside; W = 1: both column clamps collapse onto the lane's own piece
    "row": ((1, 5, 32), ((DW,), BNR, (DW,), BNR, ("dense", 4)), 2),
    "col": ((5, 1, 32), ((DW,), BNR, (DW,), BNR, ("dense", 4)), 2),
}
LOOPING = (("halo_f32_slots", 3),)
CHUNK_FORMULA = (("wg_target", 256),)
PW1, PW0 = (("pw", 1),), (("pw", 0),)
BOTH = ("fp32", "bf16")

# (net, precision, options of the device run).  fp32 and bf16 modes run the same depthwise kernels, so of the band nets only bands16 and
# seam16 run in both (the dense head and the operand copies differ); the smallest maps run in fp32
RUNS = ([("bands16", p, o) for p in BOTH for o in ((), LOOPING)] + [("band32", "fp32", ()), ("bands32", "fp32", ())]
        + [("seam16", p, ()) for p in BOTH] + [("whole32", "fp32", CHUNK_FORMULA), ("seam32", "fp32", ())]
        + [("quads", p, o) for p in BOTH for o in ((), LOOPING)]
        + [("chain", p, o) for p in BOTH for o in (PW1, PW0)]
        + [("limit32", "fp32", PW1), ("limit16", "bf16", PW1)]
        + [("neck", p, o) for p in BOTH for o in (PW1, PW0)]
        + [("sepdown", p, ()) for p in BOTH] + [("sepdown2", p, PW1) for p in BOTH]
        + [("s2x2", "fp32", ()), ("dw1x1", "fp32", PW1), ("row", "fp32", ()), ("col", "fp32", ())])


def run_id(run):
    name, precision, options = run
    return "-".join([name, precision] + [f"{k}{v}" for k, v in options])


# ---- what the plan must say (tests/test_convnet_kinds_forms_plan.py reads it from the plan's own lines)
# net: (th, bands, slabs, tiles) of its depthwise layers' forward and input-gradient launches
DW_TILES = {"bands16": (16, 2, 2, 1024), "band32": (32, 1, 2, 1024), "bands32": (32, 2, 2, 1024),
            "seam16": (16, 2, 1, 1024), "whole32": (32, 1, 1, 1024), "seam32": (32, 2, 1, 1024), "quads": (8, 2, 2, 8)}
# net: (M, the weight gradient's chunks, pixels per chunk) under the run's options
DW_CHUNKS = {"bands16": (56320, 440, 128), "band32": (71680, 280, 256), "bands32": (46080, 360, 128),
             "seam16": (30720, 240, 128), "whole32": (57344, 224, 256), "seam32": (36864, 288, 128), "quads": (220, 2, 128)}
# net: NT of k_pw, forward launches in layer order, then the gated input gradients in launch order (pw = 1, either precision)
PW_NT = {"chain": ([6, 2, 7, 2, 5, 3, 1], [3, 5, 2, 7, 2, 6])}
# the band nets whose ReLU maps must hold no pre-activation within TIE of zero, with the elements of one map
LARGE = {"bands16": 256 * 20 * 11 * 96, "band32": 512 * 28 * 5 * 256, "bands32": 256 * 36 * 5 * 256,
         "seam16": 512 * 20 * 3 * 32, "whole32": 1024 * 28 * 2 * 32, "seam32": 512 * 36 * 2 * 32}
TIE = 1e-6
# the nets whose rows barely differ behind the average pool (means over 56 to 220 pixels of 256 to 1024 rows): the logits layer carries the
# biases linspace(-4.5, 4.5), as net d of every kind file
SPREAD = tuple(LARGE)

# bands16 and band32 once more as small-integer nets (_dw_ref.exact_case on their maps and batches), where no tolerance comes in: |a2| <= 192
# by _dw_ref's argument, logits below 21120 * 192 + 3 and 35840 * 192 + 3 < 2^24.  (net, options): bands16 also on three looping workgroups
EXACT = {name: (NETS[name][0], X_SPEC[1], NETS[name][2]) for name in ("bands16", "band32")}
EXACT_RUNS = [("bands16", ()), ("bands16", LOOPING), ("band32", ())]

# per net the seeds of its parameters and of its batch, chosen from the twin alone; the CPU file asserts per net and precision the margin
# condition of _twin_checks.compare, that the bf16-operand twin agrees with itself in float32, and for LARGE that no pre-activation of a
# ReLU map lies within TIE of zero (the smallest found is beside the seed)
SEEDS = {
    # the wide nets: the first seeds at which the margin condition holds (bands16: in bf16 too); their ReLU gates by NUDGES below
    "bands16": (4, 5), "band32": (6, 7), "bands32": (4, 5),
    # smallest |pre-activation| 1.6e-6 / 2.2e-6 / 2.6e-6.  Few seeds pass TIE on both maps, and of those few the bf16 margin of seam16: 4 x 2e-2
    # of a scale near 5 is 0.4 of the 1.0 between neighbouring biases, in every one of 512 rows
    "seam16": (544, 545), "whole32": (54, 55), "seam32": (278, 279),
    "quads": (0, 1), "chain": (6, 7), "limit32": (0, 1), "limit16": (8, 9),
    "neck": (4, 5), "sepdown": (0, 1), "sepdown2": (6, 7), "row": (0, 1), "col": (0, 1),
    # batch normalisation over the TWO rows of a 1 x 1 map at B = 2: where a channel's two values lie close, 1 / sqrt(var + eps) is in the
    # hundreds and the convolution's dZ (zero-sum per channel) is cancellation noise times that.  At most seeds the twin run in float32
    # misses its own float64 self at the fp32 bound; at these it stays within 0.07 of every allowance (the CPU file asserts 0.3)
    "s2x2": (226, 227), "dw1x1": (16, 17),
}


# net: {(bn_relu layer, channel): k}: beta + k * 1e-5 (see the header).  Printed by tools/kinds_nudges.py, a loop over the twin's training
# forward on the parameters of SEEDS: every channel of either ReLU map with a pre-activation within 2e-6 of zero gets one more step, until
# there is none (2, 3 and 5 rounds).  After a change to SEEDS or to random_params the CPU file's tie test fails: run the tool and paste
NUDGES = {
    "bands16": {
        (1, 13): 1, (1, 25): 1, (1, 36): 2, (1, 39): 2, (1, 59): 1, (1, 60): 1, (1, 64): 2, (1, 70): 1, (1, 74): 1, (1, 87): 1, (1, 90): 1, (1, 93): 1,
        (3, 18): 1, (3, 21): 1, (3, 25): 1, (3, 35): 1, (3, 56): 2, (3, 63): 1, (3, 92): 1,
    },
    "band32": {
        (1, 15): 1, (1, 19): 2, (1, 22): 1, (1, 35): 1, (1, 37): 1, (1, 40): 1, (1, 60): 1, (1, 65): 1, (1, 78): 2, (1, 80): 1, (1, 83): 1, (1, 85): 1,
        (1, 97): 1, (1, 104): 1, (1, 127): 1, (1, 130): 2, (1, 138): 1, (1, 141): 1, (1, 148): 1, (1, 152): 1, (1, 154): 1, (1, 164): 2, (1, 183): 1,
        (1, 188): 1, (1, 190): 1, (1, 204): 1, (1, 212): 1, (1, 215): 2, (1, 217): 1, (1, 221): 1, (1, 236): 1, (1, 252): 1, (3, 4): 2, (3, 5): 2,
        (3, 22): 1, (3, 26): 1, (3, 42): 1, (3, 45): 1, (3, 50): 1, (3, 71): 1, (3, 72): 1, (3, 78): 1, (3, 79): 2, (3, 83): 1, (3, 84): 1, (3, 89): 1,
        (3, 95): 1, (3, 117): 1, (3, 120): 1, (3, 125): 1, (3, 133): 1, (3, 155): 1, (3, 161): 1, (3, 166): 1, (3, 173): 1, (3, 181): 1, (3, 186): 2,
        (3, 191): 1, (3, 202): 1, (3, 215): 2, (3, 218): 1, (3, 230): 1, (3, 235): 1, (3, 236): 1, (3, 241): 1, (3, 250): 1, (3, 251): 1, (3, 252): 1,
    },
    "bands32": {
        (1, 5): 1, (1, 21): 1, (1, 31): 1, (1, 39): 2, (1, 55): 1, (1, 82): 1, (1, 95): 1, (1, 106): 1, (1, 113): 1, (1, 116): 3, (1, 121): 1,
        (1, 125): 1, (1, 131): 1, (1, 133): 1, (1, 138): 1, (1, 175): 1, (1, 185): 1, (1, 188): 1, (1, 200): 1, (1, 239): 2, (3, 29): 1, (3, 32): 1,
        (3, 52): 1, (3, 61): 1, (3, 62): 2, (3, 99): 1, (3, 109): 1, (3, 116): 3, (3, 129): 1, (3, 163): 1, (3, 167): 1, (3, 175): 1, (3, 190): 1,
        (3, 200): 1, (3, 213): 1, (3, 227): 1, (3, 244): 1,
    },
}


# the twin's own float32 distance on the bias gradient of the two depthwise layers of the wide nets, measured with the twin run in float32
# against itself in float64 (gradients call): {net: {layer with parameters: max |d|}}.  That gradient is zero in exact arithmetic (batch
# normalisation follows; the float64 twin leaves 1e-14 or less), so it is held at the floor scale 1e-3, allowance 2e-4 x 1e-3 + 1e-6 = 1.2e-6,
# and torch's float32 sum over 46080 to 71680 pixels comes to 0.09 to 1.06 of that.  Only tests/test_convnet_kinds_forms_plan.py's self-distance test
# uses it: it asserts the measurement and gives these tensors the larger of the bound and four times it.  The GPU comparison widens nothing
TWIN_F32_DISTANCE = {
    "bands16": {0: 4.68e-07, 2: 1.267e-06},
    "band32": {0: 7.84e-07, 2: 6.90e-07},
    "bands32": {0: 6.09e-07, 2: 1.04e-07},
}


def case(name, seeds=None):
    """(parameters, x, y) of net `name` from its SEEDS (or from `seeds`: then without NUDGES)"""
    in_shape, layers, B = NETS[name]
    seeds = seeds or SEEDS[name]
    flat = random_params(np.random.default_rng(seeds[0]), in_shape, layers)
    if name in SPREAD:
        flat[tensor_slices(in_shape, layers)[-1][1]] = np.linspace(-4.5, 4.5, layers[-1][1]).astype(np.float32)
    if seeds == SEEDS[name]:
        for (layer, c), k in NUDGES.get(name, {}).items():
            assert layers[layer] == BNR, (name, layer)
            flat[tensor_slices(in_shape, layers)[layer][1].start + c] += np.float32(k * 1e-5)      # (no parameter-free layer in front of it)
    rng = np.random.default_rng(seeds[1])
    return flat, rng.standard_normal((B,) + in_shape).astype(np.float32), rng.integers(0, layers[-1][1], B).astype(np.int32)


def twin(name, precision, flat, **kw):
    in_shape, layers, _ = NETS[name]
    return KindsNet(in_shape, layers, flat, operand="bf16" if precision == "bf16" else "f64", **kw)


class KindsNet(DwNet):
    """DwNet with three MUTANTS of the forms this table is about, never a model of the library:
    band_seam = th -- the row above the first row of every band of th rows after the first is read as zeros (a band that does not fetch its
    upper halo row from the neighbouring band);
    stale_quad -- the pieces of a row's second slab (piece = w C / 4 + quad >= 256) use the weights and bias of the quad their lane held in
    the first slab, (quad - 256) mod C / 4 (a weight cache that is not keyed by the quad);
    swap_tiles -- a 1x1 layer of 64 or more columns stores its first two 32-column accumulator tiles in each other's place."""

    def __init__(self, in_shape, layers, flat, band_seam=0, stale_quad=False, swap_tiles=False, **kw):
        super().__init__(in_shape, layers, flat, **kw)
        self.band_seam, self.stale_quad, self.swap_tiles = band_seam, stale_quad, swap_tiles

    def _conv(self, m, t):
        torch = self.torch
        F = torch.nn.functional
        y = super()._conv(m, t)
        if m.groups != 1 and self.band_seam:
            lost = torch.zeros_like(y)
            for h0 in range(self.band_seam, t.shape[2], self.band_seam):          # what row h0 - 1 gives row h0: the taps kh = 0
                lost[:, :, h0:h0 + 1] = F.conv2d(t[:, :, h0 - 1:h0], m.weight[:, :, 0:1, :], None, padding=(0, 1), groups=m.groups)
            return y - lost
        if m.groups != 1 and self.stale_quad:
            C, Wd = m.groups, t.shape[3]
            held = (torch.arange(C) - 4 * (256 % (C // 4))) % C                    # channel c computes with the parameters of channel held[c]
            stale = F.conv2d(t, m.weight[held], m.bias[held], padding=1, groups=C)
            piece = torch.arange(Wd)[None, :] * (C // 4) + torch.arange(C)[:, None] // 4      # [c][w]
            return torch.where((piece >= 256)[None, :, None, :], stale, y)
        if m.groups == 1 and m.kernel_size == (1, 1) and self.swap_tiles and m.out_channels >= 64:
            return y[:, torch.cat([torch.arange(32, 64), torch.arange(0, 32), torch.arange(64, m.out_channels)])]
        return y
