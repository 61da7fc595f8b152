// convnet_select.hpp -- Track X: WHICH kernel runs a layer, and which launches make a step's update (Recipe, select_update, describe_update
// at the end).  Host functions only, pure: no launch, no runtime call, no allocation, every input const.  rcn_hipx_api.hip launches what
// these choose (one switch per launcher), the plan prints it (describe...), and the layer walk asks the same selectors what it needs to
// know of a neighbouring layer.
#pragma once

#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <string>

#include "../../include/rcn_hipx.h"
#include "convnet.hpp"
#include "convnet_bf16.hpp"
#include "convnet_halo.hpp"
#include "convnet_pw.hpp"
#include "convnet_dw.hpp"

namespace rcnx {

// Kernel-selection knobs, PER NET (round 4; before, most were read from the environment into function-local statics at first use:
// frozen process-wide, two nets of one process could not differ, and rcn_hipx_plan reported whatever the first call had latched).
// The environment variable of the same meaning only seeds the default when a net (or a plan) is created.
struct XOptions {
    int halo = 1;             // "halo"            RCN_HIPX_HALO            bf16: the LDS-tiled 3x3 kernels (0: implicit GEMM only)
    int bf16_pipe = 1;        // "bf16_pipe"       RCN_HIPX_BF16_PIPE       bf16: the software-pipelined LDS-tiled kernel (k_conv3x3_halo_bf16p)
    int bf16_1cb = 1;         // "bf16_1cb"        RCN_HIPX_BF16_1CB        bf16: the resident-weights form for 32-channel layers
    int bf16_rows16 = 0;      // "bf16_rows16"     RCN_HIPX_BF16_ROWS16     bf16 storage: 16 x 16 pixel blocks (two row groups per wave) where the map's height allows
    int halo_wgrad = 1;       // "halo_wgrad"      RCN_HIPX_HALO_WGRAD      the LDS-tiled weight-gradient kernels
    int fuse_pool_bwd = 1;    // "fuse_pool_bwd"   RCN_HIPX_FUSE_POOL_BWD   gradient kernels unpool while staging (no k_pool_bwd)
    int head = 1;             // "head"            RCN_HIPX_HEAD            the classifier head as one launch (k_head_f32)
    int xcd_remap = 0;        // "xcd_remap"       RCN_HIPX_XCD_REMAP       implicit-GEMM weight gradient: XCD-aware block order
    int pix_per_chunk = 0;    // "pix_per_chunk"   RCN_HIPX_PIX_PER_CHUNK   pixels per weight-gradient chunk (0: by the workgroup target)
    int wg_target = 4096;     // "wg_target"       RCN_HIPX_WG_TARGET       workgroups aimed at by the implicit-GEMM weight gradient
    int wgh_f32_target = 512; // "wgh_f32_target"  RCN_HIPX_WGH_F32_TARGET  ... by the fp32 LDS-tiled weight gradient
    int wgh_target = 256;     // "wgh_target"      RCN_HIPX_WGH_TARGET      ... by the bf16 LDS-tiled weight gradient
    int wgb_policy = 1;       // "wgb_policy"      RCN_HIPX_WGB_POLICY      bf16 implicit-GEMM weight gradient: narrower tiles / shorter chunks below 2 waves per SIMD
    int wgf_policy = 1;       // "wgf_policy"      RCN_HIPX_WGF_POLICY      fp32: the same
    int halo_f32_slots = 0;   // "halo_f32_slots"  RCN_HIPX_HALO_F32_SLOTS  resident workgroups assumed for the looping kernels (0: asked from the runtime)
    int pw = 0;               // "pw"              RCN_HIPX_PW              1x1 convolution: 1 = the streaming kernel k_pw, 0 = the implicit-GEMM form (the default in both
                              //                                            precisions: measured faster over the cifar_bottleneck step)
};
struct XOptDesc { const char* name; const char* env; int XOptions::*field; int lo, hi; };
inline const XOptDesc kXOptTable[] = {
    {"halo", "RCN_HIPX_HALO", &XOptions::halo, 0, 1},
    {"bf16_pipe", "RCN_HIPX_BF16_PIPE", &XOptions::bf16_pipe, 0, 1},
    {"bf16_1cb", "RCN_HIPX_BF16_1CB", &XOptions::bf16_1cb, 0, 1},
    {"bf16_rows16", "RCN_HIPX_BF16_ROWS16", &XOptions::bf16_rows16, 0, 1},
    {"halo_wgrad", "RCN_HIPX_HALO_WGRAD", &XOptions::halo_wgrad, 0, 1},
    {"fuse_pool_bwd", "RCN_HIPX_FUSE_POOL_BWD", &XOptions::fuse_pool_bwd, 0, 1},
    {"head", "RCN_HIPX_HEAD", &XOptions::head, 0, 1},
    {"xcd_remap", "RCN_HIPX_XCD_REMAP", &XOptions::xcd_remap, 0, 1},
    {"pix_per_chunk", "RCN_HIPX_PIX_PER_CHUNK", &XOptions::pix_per_chunk, 0, 1 << 20},
    {"wg_target", "RCN_HIPX_WG_TARGET", &XOptions::wg_target, 1, 1 << 20},
    {"wgh_f32_target", "RCN_HIPX_WGH_F32_TARGET", &XOptions::wgh_f32_target, 1, 1 << 20},
    {"wgh_target", "RCN_HIPX_WGH_TARGET", &XOptions::wgh_target, 1, 1 << 20},
    {"wgb_policy", "RCN_HIPX_WGB_POLICY", &XOptions::wgb_policy, 0, 1},
    {"wgf_policy", "RCN_HIPX_WGF_POLICY", &XOptions::wgf_policy, 0, 1},
    {"halo_f32_slots", "RCN_HIPX_HALO_F32_SLOTS", &XOptions::halo_f32_slots, 0, 1 << 20},
    {"pw", "RCN_HIPX_PW", &XOptions::pw, 0, 1},
};
inline void seed_options(XOptions& o) {
    for (const XOptDesc& d : kXOptTable) {
        const char* e = std::getenv(d.env);
        if (!e || !*e) continue;
        const long long v = std::atoll(e);
        if (v >= d.lo && v <= d.hi) o.*(d.field) = (int)v;
    }
}

// Everything selection reads of a net (rcn_hipx_net derives from it: the selectors take `const Selection&` and can reach nothing else).
struct Selection {
    XOptions opt;
    int precision = RCN_HIPX_FP32;          // GEMM operand precision of forward / dgrad (rcn_hipx_set_precision)
    // RCN_HIPX_BF16_STORED: bf16 operands AND the convolutional stage's activations / gradients (every conv and pool layer's out and dout)
    // kept in memory as bf16.  precision == RCN_HIPX_BF16 then too: what is ROUNDED does not change, only where.
    bool store16 = false;
    int tiling = RCN_HIPX_TILING_AUTO;      // fp32 3x3 kernels: implicit GEMM only / by shape / LDS-tiled wherever they apply (rcn_hipx_set_tiling)
};

// Storage of a launch's tensors (RCN_HIPX_BF16_STORED): x16 -- the input X (and a pooled-resolution input) is bf16; y16 -- the output Y and
// epilogue 3's gate tensor (both belong to the layer below in the input-gradient pass) are bf16.  The host passes every tensor as
// float*; the launch sites cast.  (launch_wgrad: x16 -- X is a bf16 tensor; y16 -- dZ, and a pooled-resolution dZ, is.)
struct Store { bool x16 = false, y16 = false; };
inline const char* const kStoreGap = "bf16 storage (RCN_HIPX_BF16_STORED) covers nets whose convolutions run on the LDS-tiled kernels with fused pooling: this layer does not (rcn_hipx_plan shows the kernels chosen)";

inline std::string strf(const char* fmt, ...) {
    char buf[512];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof buf, fmt, ap);
    va_end(ap);
    return buf;
}

// split-K factor of the implicit-GEMM kernels: few output tiles and a long contraction
inline int splitk_z(long long M, int Cout, int bn, int nkt) {
    const long long tiles = ((M + kBM - 1) / kBM) * (Cout / bn);
    int Z = 1;
    if (tiles < 256 && nkt >= 8) { Z = (int)(512 / tiles); if (Z > nkt / 4) Z = nkt / 4; if (Z < 1) Z = 1; }
    // every partial is summed by ONE thread per element in k_splitk_epilogue: 392 of them on a 128 x 32 output (the 50176 -> 10 layer of the
    // 224 x 224 net) made that kernel 101 us for 4096 sums
    if (Z > 64) Z = 64;
    return Z;
}

// Pixel-block geometry of the fp32 LDS-tiled kernels for an H x W map: 8 x 16 blocks of one image, or 8 x 8 blocks of two images
// side by side where that wastes fewer MFMA rows (8-, 24-, 56-pixel-wide maps).  Not used when less than 70 % of a block's rows
// are real pixels (the implicit-GEMM kernels have no such waste).
struct HaloPlan { bool ok; int tw; };
inline HaloPlan halo_plan(const Selection& sel, const ConvShape& s) {
    const double uh = (double)s.H / ((s.H + 7) / 8 * 8);
    const double u16 = (double)s.W / ((s.W + 15) / 16 * 16);
    const double u8 = (double)s.W / ((s.W + 7) / 8 * 8) * ((double)s.N / ((s.N + 1) / 2 * 2));
    const int tw = u8 > u16 ? 8 : 16;
    // the LDS-tiled kernels address with 32-bit element offsets
    const bool fits = (long long)(s.N + 1) * s.H * s.W * (s.Cin > s.Cout ? s.Cin : s.Cout) < 0x7fffffffLL;
    return HaloPlan{fits && (sel.tiling == RCN_HIPX_TILING_LDS || uh * (tw == 8 ? u8 : u16) >= 0.7), tw};
}
// the first layer's own kernels (k_conv1_*_f32): 1 or 3 input channels
inline bool conv1_f32_shape(const Selection& sel, const ConvShape& s) { return sel.tiling != RCN_HIPX_TILING_GEMM && (s.Cin == 1 || s.Cin == 3) && s.Cout % 32 == 0 && halo_plan(sel, s).ok; }
inline bool conv_halo_f32_shape(const Selection& sel, const ConvShape& s) { return sel.tiling != RCN_HIPX_TILING_GEMM && s.Cin % 32 == 0 && s.Cout % 32 == 0 && halo_plan(sel, s).ok; }

// does the 2x2 max-pool that follows this 3x3 convolution run in the convolution kernel's epilogue (EPI 4: LDS-tiled kernels only)?
// An INPUT of the selection -- forward() asks before it requests epilogue 4 -- that has to match select_conv's rule below: with epilogue 4
// (no split-K) every shape this accepts reaches an LDS-tiled family there.
inline bool conv_pool_fusable(const Selection& sel, const ConvShape& s) {
    if (s.H % 2 || s.W % 2) return false;
    if (conv1_f32_shape(sel, s)) return true;                          // the first layer's kernels serve both precisions
    if (sel.precision == RCN_HIPX_BF16) return sel.opt.halo != 0 && (s.Cin == 32 || s.Cin % 64 == 0);
    return conv_halo_f32_shape(sel, s);
}

// ---- forward / input gradient: Y = act(conv(X) + b); `ks` = 1 or 3; epi 0 raw / 1 bias / 2 bias + relu / 3 gate (input gradient) /
// 4 bias + ReLU + the following 2x2 max-pool (LDS-tiled kernels only: callers ask conv_pool_fusable() first) ----------------------------
enum class ConvKernel {
    conv1_fwd_f32,          // k_conv1_fwd_f32: the first layer (1 or 3 input channels), either precision
    halo_f32,               // k_conv3x3_halo_f32
    halo_bf16p,             // k_conv3x3_halo_bf16p
    halo_bf16p_rows16,      // k_conv3x3_halo_bf16p<..., __bf16, 2>: 16 x 16 pixel blocks
    halo_bf16_1cb,          // k_conv3x3_halo_bf16_1cb
    halo_bf16,              // k_conv3x3_halo_bf16
    fwd_bf16,               // k_conv_fwd_bf16 (implicit GEMM)
    fwd_bf16_map,           // k_conv_fwd_bf16 with a bf16 tensor on one side (the dense layer on top of a bf16-stored convolutional stage)
    fwd_f32,                // k_conv_fwd (implicit GEMM)
};
inline bool lds_tiled(ConvKernel k) { return k != ConvKernel::fwd_bf16 && k != ConvKernel::fwd_bf16_map && k != ConvKernel::fwd_f32; }

struct ConvChoice {
    ConvKernel kernel = ConvKernel::fwd_f32;
    const char* error = nullptr;    // or: the layer cannot run (status -3 with this message)
    bool bf16 = false;              // operands rounded to bf16: needs the transposed bf16 copy of the weights
    bool smallc = false;            // the per-element gather loader: only where a k-tile is not 32 whole channels
    int bn = 32;                    // the kernel's column-block width
    int Z = 1, kepi = 0;            // split-K factor (> 1: raw partials into the split-K slab, k_splitk_epilogue applies the epilogue), the kernel's own epilogue
    int tile_w = 0;                 // fp32 LDS-tiled kernels: pixel-block width (8: two images side by side, or 16)
    int tiles_w = 0, tiles_h = 0;   // LDS-tiled kernels: pixel blocks across and down a map
    long long items = 0;            // looping kernels: work items (pixel block, column block)
    Store st;                       // which of the launch's tensors are bf16
};

inline ConvChoice select_conv(const Selection& sel, const ConvShape& s, int ks, int epi, bool pooled_in, bool force_fp32, Store st) {
    ConvChoice c;
    const auto refuse = [&c](const char* why) { c.error = why; return c; };
    const long long M = (long long)s.N * s.H * s.W;
    c.st = st;
    c.smallc = ks * ks * s.Cin <= 32 && s.Cin % 32 != 0;
    if (!c.smallc && s.Cin % 32) return refuse("input channels must be a multiple of 32 (or the whole 3x3xCin patch <= 32)");
    if (s.Cout % 32) return refuse("output channels must be a multiple of 32");
    // bf16 mode rounds the operands of every GEMM EXCEPT the first layer's (its whole 3 x 3 x Cin patch is one k-block: nothing of the
    // MFMA rate to gain, and its own fp32 kernels are the fast ones) and the fused classifier head's (head_fusable)
    c.bf16 = sel.precision == RCN_HIPX_BF16 && !(ks == 3 && c.smallc) && !force_fp32;
    c.bn = (c.bf16 && s.Cout % 128 == 0) ? 128 : (s.Cout % 64 == 0) ? 64 : 32;
    const int nkt = c.smallc ? 1 : ks * ks * s.Cin / 32;
    // Few output tiles and a long contraction (the dense layers: M = batch) -> split-K over gridDim.z.  Not with the fused pool; not a
    // 3x3 layer under bf16 storage (whatever the batch size, it stays on the LDS-tiled kernels, the ones that take bf16 tensors); not
    // where fp32 LDS tiling is forced (the LDS-tiled kernels have no split-K form)
    c.Z = (epi == 4 || (sel.store16 && ks == 3)) ? 1
        : (!c.bf16 && ks == 3 && !c.smallc && sel.tiling == RCN_HIPX_TILING_LDS && conv_halo_f32_shape(sel, s)) ? 1 : splitk_z(M, s.Cout, c.bn, nkt);
    c.kepi = c.Z > 1 ? 0 : epi;
    if (epi == 4 && !(ks == 3 && conv_pool_fusable(sel, s))) return refuse("internal: fused conv+pool epilogue requested for a layer the LDS-tiled kernel does not cover");
    const char* const no_pooled_in = "internal: pooled-resolution input requested for a layer the LDS-tiled kernel does not cover";
    if (c.bf16) {
        // thin 3x3 layers: the LDS-tiled kernel (one halo per 8x16 output block serves all nine taps)
        if (sel.opt.halo && ks == 3 && !c.smallc && c.Z == 1 && (s.Cin == 32 || s.Cin % 64 == 0)) {
            c.bn = (s.Cout % 64 == 0) ? 64 : 32;
            c.tiles_w = (s.W + kHaloTW - 1) / kHaloTW; c.tiles_h = (s.H + kHaloTH - 1) / kHaloTH;
            if (sel.opt.bf16_pipe && (long long)(s.N + 1) * s.H * s.W * (s.Cin > s.Cout ? s.Cin : s.Cout) < 0x7fffffffLL) {
                // the pipelined form (convnet_halo_bf16.hpp): work items (pixel block, column block) on a resident grid, operands loaded a
                // phase ahead; same LDS images, rounding and MFMA order as k_conv3x3_halo_bf16 below
                c.items = (long long)c.tiles_w * c.tiles_h * s.N * (s.Cout / c.bn);
                if (st.x16 != st.y16) return refuse(kStoreGap);
                // one channel block and one 32-wide column tile: all nine taps' weights stay in LDS (with a 64-wide tile the 46 KB of weights
                // cost a third workgroup per CU: measured 190 vs 158 us on the 32 -> 64 layer of the 224 x 224 net)
                const bool onecb = s.Cin == 32 && sel.opt.bf16_1cb && c.bn == 32;
                // 16 x 16 pixel blocks (k_conv3x3_halo_bf16p<..., MG = 2>): bf16 tensors, 64-wide column blocks, a height that 16-row blocks
                // cover with no more padding than 8-row blocks do, and still at least one item per resident workgroup
                const int th2 = (s.H + 15) / 16;
                const long long items2 = (long long)c.tiles_w * th2 * s.N * (s.Cout / c.bn);
                if (sel.opt.bf16_rows16 && st.x16 && c.bn == 64 && !onecb && th2 * 16 == c.tiles_h * kHaloTH && items2 >= 512) {
                    c.kernel = ConvKernel::halo_bf16p_rows16; c.tiles_h = th2; c.items = items2;
                    return c;
                }
                if (c.items <= 0x7fffffffLL) {
                    c.kernel = onecb ? ConvKernel::halo_bf16_1cb : ConvKernel::halo_bf16p;
                    return c;
                }
            }
            if (st.x16 || st.y16) return refuse(kStoreGap);
            c.kernel = ConvKernel::halo_bf16;
            return c;
        }
        if (pooled_in) return refuse(no_pooled_in);
        if (st.x16 || st.y16) {
            // the dense layer on top of the convolutional stage: its forward pass and weight gradient READ a bf16 map, its input gradient
            // WRITES one (gated by the map, epilogue 3, or raw into a pooled gradient, epilogue 0).  A split-K launch leaves float partials.
            if (ks != 1 || c.smallc || (st.x16 && st.y16)) return refuse(kStoreGap);
            c.kernel = ConvKernel::fwd_bf16_map;
            return c;
        }
        c.kernel = ConvKernel::fwd_bf16;
        return c;
    }
    const bool first = ks == 3 && c.smallc && (epi == 2 || epi == 4) && conv1_f32_shape(sel, s);
    if (st.x16 || (st.y16 && !first)) return refuse(kStoreGap);
    if (first || (ks == 3 && !c.smallc && c.Z == 1 && conv_halo_f32_shape(sel, s))) {
        // convnet_halo.hpp.  First layer: weights in registers, the block's input halo in LDS, 32-wide column blocks; the others: one
        // staged halo per block of 128 output pixels serves all nine taps.  Work items = (pixel block, bn-wide column block); at most as
        // many workgroups as the chip holds at once (three per CU), each taking items blockIdx.x, + gridDim.x, ...
        c.kernel = first ? ConvKernel::conv1_fwd_f32 : ConvKernel::halo_f32;
        if (first) c.bn = 32;
        c.tile_w = halo_plan(sel, s).tw;
        const int nimg = 16 / c.tile_w;
        c.tiles_w = (s.W + c.tile_w - 1) / c.tile_w; c.tiles_h = (s.H + 7) / 8;
        c.items = (long long)c.tiles_w * c.tiles_h * ((s.N + nimg - 1) / nimg) * (s.Cout / c.bn);
        if (c.items > 0x7fffffffLL) return refuse("too many pixel blocks in one layer");
        return c;
    }
    if (pooled_in) return refuse(no_pooled_in);
    c.kernel = ConvKernel::fwd_f32;
    return c;
}

// one line of the plan: the launch (or launches) a choice stands for
inline std::string describe(const ConvChoice& c, const ConvShape& s, int ks, int epi, bool pooled_in) {
    const std::string head = strf("  %s %dx%dx%d->%d epi %d%s: ", ks == 3 ? "conv3x3" : "dense", s.H, s.W, s.Cin, s.Cout, epi, pooled_in ? " pooled-in" : "");
    const std::string splitk = c.Z > 1 ? " split-K " + std::to_string(c.Z) + " + k_splitk_epilogue" : "";
    const char* loader = c.smallc ? "gather" : "tile";
    switch (c.kernel) {
    case ConvKernel::conv1_fwd_f32: return head + strf("k_conv1_fwd_f32<%d, %d>, %lld items", s.Cin, c.tile_w, c.items);
    case ConvKernel::halo_f32: return head + strf("k_conv3x3_halo_f32<%d, %d>, %lld items", c.tile_w, c.bn, c.items);
    case ConvKernel::halo_bf16p_rows16: return head + strf("k_conv3x3_halo_bf16p (16 x 16 pixel blocks), %lld items", c.items);
    case ConvKernel::halo_bf16p: return head + strf("k_conv3x3_halo_bf16p, %lld items", c.items);
    case ConvKernel::halo_bf16_1cb: return head + strf("k_conv3x3_halo_bf16_1cb<32>, %lld items", c.items);
    case ConvKernel::halo_bf16: return head + "k_conv3x3_halo_bf16";
    case ConvKernel::fwd_bf16_map: return strf("  dense %d->%d epi %d: k_conv_fwd_bf16<1, tile, %d>", s.Cin, s.Cout, epi, c.bn) + splitk + (c.st.x16 ? ", bf16 input map" : ", bf16 output map");
    case ConvKernel::fwd_bf16: return head + strf("k_conv_fwd_bf16<%d, %s, %d>", ks, loader, c.bn) + splitk;
    case ConvKernel::fwd_f32: return head + strf("k_conv_fwd<%d, %s, %d>", ks, loader, c.bn) + splitk;
    }
    return head;
}
// does an LDS-tiled kernel run this 3x3 convolution (the layer walk asks this of a layer's INPUT-GRADIENT call)?
inline bool conv_halo_runs(const Selection& sel, const ConvShape& s) {
    const ConvChoice c = select_conv(sel, s, 3, 0, false, false, Store{});
    return !c.error && lds_tiled(c.kernel);
}

// ---- weight gradient: partial [W | b] tiles, one per chunk of pixels, into the layer's slab ---------------------------------------------
enum class WgradKernel {
    conv1_wgrad_f32,        // k_conv1_wgrad_f32: the first layer, either precision
    halo_f32,               // k_wgrad3x3_halo_f32
    halo_bf16,              // k_wgrad3x3_halo_bf16
    wgrad_bf16,             // k_conv_wgrad_bf16 (implicit GEMM)
    wgrad_f32,              // k_conv_wgrad (implicit GEMM)
};
inline bool lds_tiled(WgradKernel k) { return k != WgradKernel::wgrad_bf16 && k != WgradKernel::wgrad_f32; }

struct WgradChoice {
    WgradKernel kernel = WgradKernel::wgrad_f32;
    const char* error = nullptr;    // or: the layer cannot run (status -3 with this message)
    bool smallc = false;            // the per-element gather loader
    int cb = 32, bn = 32;           // input-channel block (k_wgrad3x3_halo_bf16) and column-block width of a workgroup's tile
    int nk = 1;                     // k_conv_wgrad_bf16: waves (32-row k-blocks) per workgroup
    int ppc = 0, bpc = 0;           // a chunk: pixels (implicit GEMM) or pixel blocks (LDS-tiled)
    int chunks = 0;                 // THE chunk count: partial tiles in the slab, each (K + 1) x Cout
    int tile_w = 0;                 // fp32 LDS-tiled kernels: pixel-block width
    int tiles_w = 0, tiles_h = 0;   // LDS-tiled kernels: pixel blocks across and down a map
    long long tiles = 0;            // LDS-tiled kernels: workgroups (tiles of [W | b]) that share a chunk
};

// Pixels per weight-gradient chunk.  Every chunk costs one (K+1) x Cout partial tile written to the slab and read back by
// the reduction launch, and a chunk is worked on by `tiles` workgroups (k-blocks x n-tiles), so the chunk size aims at a
// total number of workgroups -- wide layers need few chunks -- with 1024 pixels as the floor (measured best on the small
// CIFAR / MNIST nets, where parallelism is what matters).
inline int pix_per_chunk(const Selection& sel, long long M, long long tiles) {
    const int v = sel.opt.pix_per_chunk >= 128 ? sel.opt.pix_per_chunk / 128 * 128 : 0;
    if (v) return v;
    const long long target = sel.opt.wg_target;
    long long pix = (M * tiles / target + 127) / 128 * 128;
    if (pix < 1024) pix = 1024;
    if (pix > 32768) pix = 32768;
    return (int)pix;
}

inline WgradChoice select_wgrad(const Selection& sel, const ConvShape& s, int ks, bool pooled_dz, Store st) {
    WgradChoice c;
    const auto refuse = [&c](const char* why) { c.error = why; return c; };
    const long long M = (long long)s.N * s.H * s.W;
    const int K = ks * ks * s.Cin;
    const bool bf16 = sel.precision == RCN_HIPX_BF16;
    c.smallc = K <= 32 && s.Cin % 32 != 0;
    // the family, by shape: the LDS-tiled kernels where they apply (the first layer's fp32 kernels in either precision), else implicit GEMM
    const bool lds = sel.opt.halo_wgrad && ks == 3;
    c.kernel = lds && K <= 32 && conv1_f32_shape(sel, s) ? WgradKernel::conv1_wgrad_f32
             : lds && K > 32 && !bf16 && conv_halo_f32_shape(sel, s) ? WgradKernel::halo_f32
             : lds && K > 32 && bf16 && (s.Cin == 32 || s.Cin % 64 == 0) && s.H >= kHaloTH / 2 && s.W >= kHaloTW / 2 ? WgradKernel::halo_bf16
             : bf16 && !c.smallc ? WgradKernel::wgrad_bf16 : WgradKernel::wgrad_f32;
    if (M > 0x7fff0000LL) return refuse("too many output pixels in one layer (N*H*W must stay below 2^31)");
    if (pooled_dz && !lds_tiled(c.kernel)) return refuse("internal: pooled-resolution dZ requested for a layer the LDS-tiled weight-gradient kernel does not cover");
    if (c.kernel == WgradKernel::conv1_wgrad_f32 ? st.x16 : ((st.x16 || st.y16) && !bf16)) return refuse(kStoreGap);
    const int bn0 = (s.Cout % 64 == 0) ? 64 : 32;
    switch (c.kernel) {
    case WgradKernel::conv1_wgrad_f32:
    case WgradKernel::halo_f32: {
        // first layer (convnet_halo.hpp): one 32 x 32 tile (rows = patch entries) per (co block, chunk of pixel blocks), 1024 workgroups aimed at.
        // fp32 LDS-tiled (convnet_halo.hpp): workgroup = (32 input channels, 32 output channels, chunk of pixel blocks), all nine taps.
        // Every chunk costs one (K+1) x Cout partial written and read back by the reduce whatever the number of (ci, co) workgroups
        // that share it, so: as few chunks as fill the chip twice over.
        const bool first = c.kernel == WgradKernel::conv1_wgrad_f32;
        c.tile_w = halo_plan(sel, s).tw;
        const int nimg = 16 / c.tile_w;
        c.tiles_w = (s.W + c.tile_w - 1) / c.tile_w; c.tiles_h = (s.H + 7) / 8;
        const long long blocks = (long long)c.tiles_w * c.tiles_h * ((s.N + nimg - 1) / nimg);
        c.tiles = (long long)(first ? 1 : s.Cin / 32) * (s.Cout / 32);
        long long want = ((first ? 1024 : sel.opt.wgh_f32_target) + c.tiles - 1) / c.tiles;
        if (want > blocks) want = blocks;
        if (!first && want > 32768) want = 32768;
        c.bpc = (int)((blocks + want - 1) / want);
        c.chunks = (int)((blocks + c.bpc - 1) / c.bpc);
        return c;
    }
    case WgradKernel::halo_bf16: {
        // LDS-tiled: input halo + dZ block staged once per 8x16 pixel block, nine waves = nine filter taps (convnet_halo_bf16.hpp)
        if (st.x16 != st.y16) return refuse(kStoreGap);
        c.tiles_w = (s.W + kHaloTW - 1) / kHaloTW; c.tiles_h = (s.H + kHaloTH - 1) / kHaloTH;
        const long long blocks = (long long)c.tiles_w * c.tiles_h * s.N;
        c.cb = s.Cin == 32 ? 32 : 64; c.bn = bn0;
        // Pixel blocks per chunk: every chunk costs one (K+1) x Cout partial tile written and read back by the reduce, so aim at
        // `target` workgroups in total (tiles per chunk x chunks) rather than at a fixed chunk count -- wide layers have many
        // tiles per chunk and need few chunks.
        // (256 = one per CU: the 576-thread workgroup with its 64+ accumulator registers per wave is alone on its CU anyway, and every
        // chunk fewer is a partial [W | b] less to write and reduce: synth-224 bf16 5.20 ms at 512, 5.05 at 256, 5.49 at 384 -- 1.5 per CU)
        const int target = sel.opt.wgh_target;
        c.tiles = (long long)(s.Cin / c.cb) * (s.Cout / c.bn);
        c.bpc = (int)((blocks * c.tiles + target - 1) / target);
        if (c.bpc < 8) c.bpc = blocks < 8 ? (int)blocks : 8;
        c.chunks = (int)((blocks + c.bpc - 1) / c.bpc);
        return c;
    }
    default: break;
    }
    // implicit GEMM: chunks of pixels
    c.bn = bn0;
    c.ppc = pix_per_chunk(sel, M, (long long)(c.smallc ? 1 : K / 32) * (s.Cout / bn0));
    c.chunks = (int)((M + c.ppc - 1) / c.ppc);
    if (c.kernel == WgradKernel::wgrad_bf16) {
        // bf16 operands, transposed LDS reads (convnet_bf16.hpp); NKB waves per workgroup, one 32-row k-block each
        if (st.y16 || (st.x16 && ks != 1)) return refuse(kStoreGap);
        const int nkb = K / 32;
        c.nk = nkb % 4 == 0 ? 4 : nkb % 3 == 0 ? 3 : nkb % 2 == 0 ? 2 : 1;
        // A wave owns one 32-row k-block x bn columns over the chunk's pixels, so a dense layer behind a pooled map is FEW waves (MNIST shape
        // 3136 -> 128 at B = 4096: 98 x 2 x 4 chunks = 784 on the chip's 1024 SIMDs, 62 us for 7 us of traffic).  Below two waves per SIMD
        // take 32-wide column blocks (no more slab, X re-read from L2), below one per SIMD also shorter chunks (down to 256 pixels).
        if (sel.opt.wgb_policy) {
            if ((long long)nkb * (s.Cout / c.bn) * c.chunks < 2048) c.bn = 32;
            while ((long long)nkb * (s.Cout / c.bn) * c.chunks < 1024 && c.ppc > 256) { c.ppc /= 2; c.chunks = (int)((M + c.ppc - 1) / c.ppc); }
        }
        return c;
    }
    if (st.x16 || st.y16) return refuse(kStoreGap);
    // (as in the bf16 branch above: below two waves per SIMD the column blocks are 32 wide -- CIFAR net's 2048 -> 256 at B = 512: 256 -> 512
    // workgroups, step 0.419 -> 0.417 ms; MNIST shape B = 256: 0.165 -> 0.1625 ms)
    if (sel.opt.wgf_policy && !c.smallc && 4LL * (K / 32) * (s.Cout / bn0) * c.chunks < 2048) c.bn = 32;
    return c;
}

// (on_map: a 1x1 convolution, the KS = 1 kernels with rows walking the H x W map)
inline std::string describe(const WgradChoice& c, const ConvShape& s, int ks, bool pooled_dz, bool on_map = false) {
    const std::string head = strf("  wgrad %s %dx%dx%d->%d%s: ", ks == 3 ? "conv3x3" : on_map ? "conv1x1" : "dense", s.H, s.W, s.Cin, s.Cout, pooled_dz ? " pooled-dZ" : "");
    switch (c.kernel) {
    case WgradKernel::conv1_wgrad_f32: return head + strf("k_conv1_wgrad_f32<%d, %d>, %d chunks", s.Cin, c.tile_w, c.chunks);
    case WgradKernel::halo_f32: return head + strf("k_wgrad3x3_halo_f32<%d>, %d chunks x %lld tiles", c.tile_w, c.chunks, c.tiles);
    case WgradKernel::halo_bf16: return head + strf("k_wgrad3x3_halo_bf16<%d, %d>, %d chunks x %lld tiles", c.cb, c.bn, c.chunks, c.tiles);
    case WgradKernel::wgrad_bf16: return head + strf("k_conv_wgrad_bf16<%d, %d, %d>, %d chunks", ks, c.bn, c.nk, c.chunks);
    case WgradKernel::wgrad_f32: return head + strf("k_conv_wgrad<%d, %s, %d>, %d chunks", ks, c.smallc ? "gather" : "tile", c.bn, c.chunks);
    }
    return head;
}
// does an LDS-tiled kernel run this layer's weight gradient?
inline bool wgrad_halo_runs(const Selection& sel, const ConvShape& s, int ks) { return lds_tiled(select_wgrad(sel, s, ks, false, Store{}).kernel); }

// ---- RCN_HIPX_CONV3X3_S2: all three GEMMs of a strided layer on the implicit-GEMM family, in both operand precisions.  The LDS-tiled
// (halo) families assume stride 1; these selectors take the strided shape types and hold no LDS-tiled kernel, no fused pool and no
// pooled-resolution operand to hand out -- conv_halo_runs, wgrad_halo_runs and conv_pool_fusable take a ConvShape and are never asked of
// a strided layer.
struct ConvS2Choice {
    const char* error = nullptr;    // or: the layer cannot run (status -3 with this message)
    bool bf16 = false;              // operands rounded to bf16
    int bn = 32;                    // the kernel's column-block width
    int Z = 1, kepi = 0;            // forward: split-K factor and the kernel's own epilogue, as ConvChoice's
    long long tiles = 0;            // 128-row tiles: of the output map (forward), of ONE parity class (input gradient: four classes of as many)
};
// forward: Y = conv(X) + b (epi 1).  Split-K applies as to the stride-1 kernel -- same body, M = the OUTPUT pixels: a small strided map
// has few output tiles and a contraction of 9 Cin / 32 >= 9 K-tiles
inline ConvS2Choice select_conv_s2(const Selection& sel, const ConvShapeS2& s, int epi) {
    ConvS2Choice c;
    const auto refuse = [&c](const char* why) { c.error = why; return c; };
    if (s.H % 2 || s.W % 2) return refuse("a strided convolution needs even height and width");
    if (s.Cin % 32) return refuse("a strided convolution's input channels must be a multiple of 32");
    if (s.Cout % 32) return refuse("output channels must be a multiple of 32");
    const long long M = gemm_rows(s);
    c.bf16 = sel.precision == RCN_HIPX_BF16;
    c.bn = (c.bf16 && s.Cout % 128 == 0) ? 128 : (s.Cout % 64 == 0) ? 64 : 32;
    c.Z = splitk_z(M, s.Cout, c.bn, 9 * s.Cin / 32);
    c.kepi = c.Z > 1 ? 0 : epi;
    c.tiles = (M + kBM - 1) / kBM;
    return c;
}
inline std::string describe(const ConvS2Choice& c, const ConvShapeS2& s, int epi) {
    return strf("  conv3x3/2 %dx%dx%d->%dx%dx%d epi %d: %s<3, tile, %d, ConvShapeS2>, %lld output tiles", s.H, s.W, s.Cin, s.H / 2, s.W / 2, s.Cout, epi, c.bf16 ? "k_conv_fwd_bf16" : "k_conv_fwd", c.bn, c.tiles) +
           (c.Z > 1 ? " split-K " + std::to_string(c.Z) + " + k_splitk_epilogue" : std::string(", no split-K"));
}
// input gradient: one launch over the four parity classes of input pixels (convnet.hpp), epi 0 (raw) or 3 (gated by the layer below's
// output).  No split-K: the classes' contractions differ in length.  Column blocks of 64 or 32 in either precision.
inline ConvS2Choice select_dgrad_s2(const Selection& sel, const ConvShapeS2T& s, int epi) {
    ConvS2Choice c;
    const auto refuse = [&c](const char* why) { c.error = why; return c; };
    if (s.H % 2 || s.W % 2 || s.Cin % 32 || s.Cout % 32) return refuse("internal: a strided input gradient of a shape the layer table refuses");
    if ((long long)s.N * s.H * s.W > 0x7fff0000LL) return refuse("too many input pixels in one strided layer (N*H*W must stay below 2^31)");
    c.bf16 = sel.precision == RCN_HIPX_BF16;
    c.bn = (s.Cout % 64 == 0) ? 64 : 32;
    c.kepi = epi;
    c.tiles = (gemm_rows(s) + kBM - 1) / kBM;
    return c;
}
inline std::string describe(const ConvS2Choice& c, const ConvShapeS2T& s, int epi) {
    return strf("  dgrad conv3x3/2 %dx%dx%d->%dx%dx%d epi %d: %s<3, tile, %d, ConvShapeS2T>, one launch, parity classes (odd,odd) 4 taps: %lld tiles, (odd,even) 2 taps: %lld tiles, (even,odd) 2 taps: %lld tiles, (even,even) 1 tap: %lld tiles",
                s.H / 2, s.W / 2, s.Cin, s.H, s.W, s.Cout, epi, c.bf16 ? "k_conv_fwd_bf16" : "k_conv_fwd", c.bn, c.tiles, c.tiles, c.tiles, c.tiles);
}
// weight gradient: the implicit-GEMM kernels' chunks of OUTPUT pixels; bf16: always three waves (9 Cin / 32 k-blocks)
inline WgradChoice select_wgrad_s2(const Selection& sel, const ConvShapeS2& s) {
    WgradChoice c;
    const auto refuse = [&c](const char* why) { c.error = why; return c; };
    const long long M = gemm_rows(s);
    const int nkb = 9 * s.Cin / 32;
    const bool bf16 = sel.precision == RCN_HIPX_BF16;
    c.kernel = bf16 ? WgradKernel::wgrad_bf16 : WgradKernel::wgrad_f32;
    if (s.H % 2 || s.W % 2 || s.Cin % 32 || s.Cout % 32) return refuse("internal: a strided weight gradient of a shape the layer table refuses");
    if ((long long)s.N * s.H * s.W > 0x7fff0000LL) return refuse("too many input pixels in one strided layer (N*H*W must stay below 2^31)");
    const int bn0 = (s.Cout % 64 == 0) ? 64 : 32;
    c.bn = bn0;
    c.ppc = pix_per_chunk(sel, M, (long long)nkb * (s.Cout / bn0));
    c.chunks = (int)((M + c.ppc - 1) / c.ppc);
    if (bf16) {
        c.nk = 3;
        if (sel.opt.wgb_policy) {         // (select_wgrad's policy: narrower tiles below two waves per SIMD, shorter chunks below one)
            if ((long long)nkb * (s.Cout / c.bn) * c.chunks < 2048) c.bn = 32;
            while ((long long)nkb * (s.Cout / c.bn) * c.chunks < 1024 && c.ppc > 256) { c.ppc /= 2; c.chunks = (int)((M + c.ppc - 1) / c.ppc); }
        }
        return c;
    }
    if (sel.opt.wgf_policy && 4LL * nkb * (s.Cout / bn0) * c.chunks < 2048) c.bn = 32;
    return c;
}
inline std::string describe(const WgradChoice& c, const ConvShapeS2& s) {
    const std::string head = strf("  wgrad conv3x3/2 %dx%dx%d->%dx%dx%d: ", s.H, s.W, s.Cin, s.H / 2, s.W / 2, s.Cout);
    return c.kernel == WgradKernel::wgrad_bf16 ? head + strf("k_conv_wgrad_bf16<3, %d, 3, ConvShapeS2>, %d chunks", c.bn, c.chunks) : head + strf("k_conv_wgrad<3, tile, %d, ConvShapeS2>, %d chunks", c.bn, c.chunks);
}

// ---- RCN_HIPX_CONV1X1: the forward pass (epi 1) and the input gradient (epi 0 / 3) of a 1x1 convolution on an H x W map, s.Cin the
// contraction and s.Cout the columns of the launch (the input gradient: the layer's Cout and Cin).  Option pw = 1: the streaming kernel
// k_pw (convnet_pw.hpp) -- the whole [K][nb] weight slice in LDS, nb the widest multiple of 32 that divides Cout, fits the slice and the
// accumulators, and `passes` = Cout / nb reads of the input.  Otherwise (pw = 0, the measured default; or a contraction no 32-wide slice
// holds) the implicit-GEMM form: select_conv's choice for ks = 1 on the map, split-K as splitk_z decides; `gemm` is that choice.
struct PwChoice {
    const char* error = nullptr;    // or: the layer cannot run (status -3 with this message)
    bool stream = false;            // k_pw; false: the implicit-GEMM form in `gemm`
    bool bf16 = false;              // operands rounded to bf16
    int nb = 32, passes = 1;        // k_pw: column slice and workgroup columns (reads of the input)
    long long items = 0;            // k_pw: row blocks of kPwRows rows, dealt over the resident grid
    long long grid = 0;             // k_pw: workgroups per column slice where the option halo_f32_slots fixes them (0: as many as the runtime says the chip holds)
    ConvChoice gemm;
};
inline PwChoice select_pw(const Selection& sel, const ConvShape& s, int epi) {
    PwChoice c;
    const auto refuse = [&c](const char* why) { c.error = why; return c; };
    if (s.Cin % 32 || s.Cout % 32) return refuse("a 1x1 convolution's input and output channels must be multiples of 32");
    if (epi != 0 && epi != 1 && epi != 3) return refuse("internal: a 1x1 convolution has epilogues 0, 1 and 3");
    c.bf16 = sel.precision == RCN_HIPX_BF16;
    c.items = ((long long)s.N * s.H * s.W + kPwRows - 1) / kPwRows;
    if (sel.opt.pw && (long long)s.Cin * 32 <= pw_slice_elems(c.bf16)) {
        // (64-bit row offsets in the kernel: no bound on M)
        int nt = 0;
        for (int t = 1; t <= kPwMaxNB / 32; ++t)
            if ((s.Cout / 32) % t == 0 && (long long)s.Cin * 32 * t <= pw_slice_elems(c.bf16)) nt = t;
        c.stream = true; c.nb = 32 * nt; c.passes = s.Cout / c.nb;
        if (sel.opt.halo_f32_slots > 0) { c.grid = sel.opt.halo_f32_slots / c.passes; if (c.grid < 1) c.grid = 1; if (c.grid > c.items) c.grid = c.items; }
        return c;
    }
    c.gemm = select_conv(sel, s, 1, epi, false, false, Store{});
    c.error = c.gemm.error;
    return c;
}
inline std::string describe(const PwChoice& c, const ConvShape& s, int epi) {
    const std::string head = strf("  conv1x1 %dx%dx%d->%d epi %d: ", s.H, s.W, s.Cin, s.Cout, epi);
    if (c.stream)
        return head + strf("k_pw<%s, %d>, weights [%d][%d] staged once in LDS, %lld row blocks of %d rows on %s, input read %s", c.bf16 ? "bf16" : "f32", c.nb / 32, s.Cin, c.nb,
                           c.items, kPwRows, c.grid ? (std::to_string(c.grid) + " looping workgroups per slice").c_str() : "a resident grid",
                           c.passes == 1 ? "once" : (std::to_string(c.passes) + " times (" + std::to_string(c.passes) + " column slices)").c_str());
    const int bn = c.gemm.bn;
    const long long tiles = ((long long)s.N * s.H * s.W + kBM - 1) / kBM;
    return head + strf("%s<1, tile, %d>", c.gemm.bf16 ? "k_conv_fwd_bf16" : "k_conv_fwd", bn) + (c.gemm.Z > 1 ? " split-K " + std::to_string(c.gemm.Z) + " + k_splitk_epilogue" : std::string()) +
           strf(", %d-wide column blocks, %lld row tiles, input read %d times", bn, tiles, s.Cout / bn);
}

// ---- RCN_HIPX_DWCONV3X3 (convnet_dw.hpp): the forward pass (epi 1) and the input gradient (epi 0 / 3) of a depthwise 3x3 convolution on an
// H x W map of s.Cin == s.Cout channels, fp32 in either precision mode.  A tile is (image, band of `th` rows, slab of 256 16-byte pieces of a
// row); th is the tallest of 32 / 16 / 8 that still gives the chip kDwMinTiles tiles (a taller band re-reads fewer halo rows; a
// whole-height band none), else 8.  The grid loops over the tiles: `grid` workgroups where the option halo_f32_slots fixes them,
// else (0) as many as the runtime says the chip holds.
constexpr long long kDwMinTiles = 1024;      // 256 CUs x 4 workgroups of 256 threads (k_dw holds about 100 VGPRs: four waves per SIMD)
struct DwChoice {
    const char* error = nullptr;    // or: the layer cannot run (status -3 with this message)
    int th = 8, bands = 1, slabs = 1;
    long long items = 0, grid = 0;
};
inline DwChoice select_dw(const Selection& sel, const ConvShape& s, int epi) {
    DwChoice c;
    const auto refuse = [&c](const char* why) { c.error = why; return c; };
    if (s.Cin != s.Cout) return refuse("internal: a depthwise convolution keeps its channel count");
    if (s.Cin % 32) return refuse("a depthwise convolution's channels must be a multiple of 32");
    if (epi != 0 && epi != 1 && epi != 3) return refuse("internal: a depthwise convolution has epilogues 0, 1 and 3");
    if ((long long)s.W * (s.Cin / 4) > 0x3fffffffLL) return refuse("a depthwise convolution's map row must hold fewer than 2^30 16-byte pieces");
    c.slabs = (int)(((long long)s.W * (s.Cin / 4) + kDwSlab - 1) / kDwSlab);
    c.th = 8;
    for (int th = 32; th > 8; th /= 2)
        if (th < s.H + 8 && (long long)s.N * ((s.H + th - 1) / th) * c.slabs >= kDwMinTiles) { c.th = th; break; }
    c.bands = (s.H + c.th - 1) / c.th;
    c.items = (long long)s.N * c.bands * c.slabs;
    if (sel.opt.halo_f32_slots > 0) c.grid = sel.opt.halo_f32_slots < c.items ? sel.opt.halo_f32_slots : c.items;
    return c;
}
inline std::string describe(const DwChoice& c, const ConvShape& s, int epi) {
    return strf("  dwconv 3x3 %dx%dx%d epi %d: k_dw<%d> (fp32 arithmetic), tiles of %d rows x %d pieces of 16 bytes (%d bands x %d slabs per image, %lld tiles), workgroups %s", s.H, s.W, s.Cin, epi,
                epi, c.th, kDwSlab, c.bands, c.slabs, c.items, c.grid ? (std::to_string(c.grid) + " looping over the tiles").c_str() : "a resident grid looping over the tiles");
}
// ... and its weight gradient: partial [10][C] tiles, one per chunk of `ppc` consecutive pixels, by workgroups (chunk, 32-channel group)
struct DwWgradChoice {
    const char* error = nullptr;
    int ppc = 0, chunks = 0, groups = 0;
};
inline DwWgradChoice select_dw_wgrad(const Selection& sel, const ConvShape& s) {
    DwWgradChoice c;
    if (s.Cin != s.Cout || s.Cin % 32) { c.error = "a depthwise convolution's channels must be a multiple of 32"; return c; }
    const long long M = (long long)s.N * s.H * s.W;
    c.groups = s.Cin / kDwGroup;
    // the option pix_per_chunk as for every weight gradient; else aimed at wg_target workgroups like the implicit-GEMM kernels, but with a
    // floor of 128 pixels, not their 1024: a chunk costs this kernel one [10][32] tile per workgroup (1.3 KB against 20 KB of input per
    // 128 pixels), and at 1024 the 8 x 8 x 256 map of cifar_sep was 256 workgroups for 1024 resident slots
    const int opt = sel.opt.pix_per_chunk >= 128 ? sel.opt.pix_per_chunk / 128 * 128 : 0;
    long long pix = opt ? opt : (M * c.groups / sel.opt.wg_target + 127) / 128 * 128;
    if (pix < 128) pix = 128;
    if (pix > 32768) pix = 32768;
    c.ppc = (int)pix;
    if ((M + c.ppc - 1) / c.ppc > 0x7fffffffLL) { c.error = "a depthwise weight gradient of more than 2^31 chunks"; return c; }
    c.chunks = (int)((M + c.ppc - 1) / c.ppc);
    return c;
}
inline std::string describe(const DwWgradChoice& c, const ConvShape& s) {
    return strf("  wgrad dwconv 3x3 %dx%dx%d: k_dw_wgrad (fp32 arithmetic), %d channel groups x %d chunks of %d pixels", s.H, s.W, s.Cin, c.groups, c.chunks, c.ppc);
}

// ---- RCN_HIPX_DWCONV3X3_S2 (convnet_dw_s2.hpp): the strided depthwise convolution on an even H x W map (s: the layer's INPUT map), output
// oH x oW = (H/2) x (W/2), fp32 in either precision mode.  The forward pass (epi 1) and the input gradient (epi 0 / 3) tile the same
// geometry: a tile is (image, band of `th` output rows -- for the input gradient: rows of 2 x 2 blocks of input pixels --, slab of 256
// 16-byte output pieces / blocks); th by select_dw's rule over the output rows, the grid looping over the tiles as k_dw's.
inline DwChoice dw_s2_tiles(const Selection& sel, const ConvShape& s) {
    DwChoice c;
    const auto refuse = [&c](const char* why) { c.error = why; return c; };
    if (s.Cin != s.Cout) return refuse("internal: a depthwise convolution keeps its channel count");
    if (s.Cin % 32) return refuse("a depthwise convolution's channels must be a multiple of 32");
    if (s.H % 2 || s.W % 2) return refuse("a strided convolution needs even height and width");
    if ((long long)s.W * (s.Cin / 4) > 0x3fffffffLL) return refuse("a depthwise convolution's map row must hold fewer than 2^30 16-byte pieces");
    const int oH = s.H / 2, oW = s.W / 2;
    c.slabs = (int)(((long long)oW * (s.Cin / 4) + kDwSlab - 1) / kDwSlab);
    c.th = 8;
    for (int th = 32; th > 8; th /= 2)
        if (th < oH + 8 && (long long)s.N * ((oH + th - 1) / th) * c.slabs >= kDwMinTiles) { c.th = th; break; }
    c.bands = (oH + c.th - 1) / c.th;
    c.items = (long long)s.N * c.bands * c.slabs;
    if (sel.opt.halo_f32_slots > 0) c.grid = sel.opt.halo_f32_slots < c.items ? sel.opt.halo_f32_slots : c.items;
    return c;
}
inline DwChoice select_dw_s2(const Selection& sel, const ConvShape& s, int epi) {
    DwChoice c = dw_s2_tiles(sel, s);
    if (!c.error && epi != 1) c.error = "internal: a strided depthwise convolution's forward pass has epilogue 1";
    return c;
}
inline DwChoice select_dw_s2_dgrad(const Selection& sel, const ConvShape& s, int epi) {
    DwChoice c = dw_s2_tiles(sel, s);
    if (!c.error && epi != 0 && epi != 3) c.error = "internal: a strided depthwise convolution's input gradient has epilogues 0 and 3";
    return c;
}
inline std::string dw_s2_grid_words(const DwChoice& c) { return c.grid ? std::to_string(c.grid) + " looping over the tiles" : std::string("a resident grid looping over the tiles"); }
inline std::string describe_dw_s2(const DwChoice& c, const ConvShape& s, int epi) {
    return strf("  dwconv 3x3/2 %dx%dx%d->%dx%dx%d epi %d: k_dw_s2_fwd (fp32 arithmetic), tiles of %d output rows x %d pieces of 16 bytes (%d bands x %d slabs per image, %lld tiles), workgroups %s",
                s.H, s.W, s.Cin, s.H / 2, s.W / 2, s.Cin, epi, c.th, kDwSlab, c.bands, c.slabs, c.items, dw_s2_grid_words(c).c_str());
}
inline std::string describe_dw_s2_dgrad(const DwChoice& c, const ConvShape& s, int epi) {
    return strf("  dgrad dwconv 3x3/2 %dx%dx%d->%dx%dx%d epi %d: k_dw_s2_dgrad<%d> (fp32 arithmetic), one launch, every input element written once: 2x2 blocks with 1 / 2 / 2 / 4 taps, "
                "tiles of %d block rows x %d blocks (%d bands x %d slabs per image, %lld tiles), workgroups %s",
                s.H / 2, s.W / 2, s.Cin, s.H, s.W, s.Cin, epi, epi, c.th, kDwSlab, c.bands, c.slabs, c.items, dw_s2_grid_words(c).c_str());
}
// ... and its weight gradient: select_dw_wgrad's chunking (pix_per_chunk / wg_target, the 128-pixel floor) over the OUTPUT pixels
inline DwWgradChoice select_dw_s2_wgrad(const Selection& sel, const ConvShape& s) {
    DwWgradChoice c;
    if (s.H % 2 || s.W % 2) { c.error = "a strided convolution needs even height and width"; return c; }
    return select_dw_wgrad(sel, ConvShape{s.N, s.H / 2, s.W / 2, s.Cin, s.Cout});
}
inline std::string describe_dw_s2_wgrad(const DwWgradChoice& c, const ConvShape& s) {
    return strf("  wgrad dwconv 3x3/2 %dx%dx%d->%dx%dx%d: k_dw_s2_wgrad (fp32 arithmetic), %d channel groups x %d chunks of %d output pixels", s.H, s.W, s.Cin, s.H / 2, s.W / 2, s.Cin, c.groups,
                c.chunks, c.ppc);
}

// ---- the step's update launch (convnet_update.hpp)
// what a training step does with its gradient: the whole update (a net that does not accumulate), or one micro-step of a cycle of
// rcn_hipx_set_accumulate -- the first stores into the accumulator, a middle one adds, the last adds and applies the update
enum Micro { kWholeStep = 0, kMicroFirst = 1, kMicroMiddle = 2, kMicroLast = 3 };

// Everything an update is configured with, and the dropout in front of it (rcn_hipx_net derives from it; a dry-run net copies it in one assignment, so the plan and the
// step agree by construction).  The buffers and the state these settings need stay members of the net.
struct Recipe {
    int optim = 0;                          // the optimiser selected: 0 SGD (rcn_hipx_set_sgd, the default), 1 Adam (rcn_hipx_set_adam)
    float sgd_mu = 0.f, sgd_wd = 0.f; int sgd_nesterov = 0;      // rcn_hipx_set_sgd: (0, 0, 0) is plain SGD
    // rcn_hipx_set_adam (convnet_adam.hpp): b1 = (float)beta1, b2 = (float)beta2, a1 = fl(1.0f - b1), a2 = fl(1.0f - b2); decoupled: AdamW
    float adam_b1 = 0.9f, adam_b2 = 0.999f, adam_a1 = 1.0f - 0.9f, adam_a2 = 1.0f - 0.999f, adam_eps = 1e-8f, adam_wd = 0.f; int adam_decoupled = 0;
    float loss_eps = 0.f;                   // rcn_hipx_set_loss: 0 is the hard cross-entropy through k_softmax_ce / k_head_f32<true>
    float ema_decay = 0.f;                  // rcn_hipx_set_ema: 0 is off
    float clip_max = 0.f;                   // rcn_hipx_set_clip: 0 is off
    int accum_k = 1; float accum_c = 1.f;   // rcn_hipx_set_accumulate: 1 is off; accum_c = fl(1.0f / k)
    // rcn_hipx_set_dropout (convnet_dropout.hpp): 0 is off; drop_s = fl(1.0f / fl(1.0f - p)), drop_thr = llrint(p * 2^24)
    float drop_p = 0.f; unsigned long long drop_seed = 0; float drop_s = 1.f; unsigned drop_thr = 0;
    float bn_momentum = 0.1f, bn_eps = 1e-5f;      // rcn_hipx_set_bn (convnet_bn.hpp): torch.nn.BatchNorm2d's defaults
};
inline bool adam_on(const Recipe& r) { return r.optim == 1; }
inline bool sgd_default(const Recipe& r) { return r.sgd_mu == 0.f && r.sgd_wd == 0.f && !r.sgd_nesterov; }
inline bool ema_on(const Recipe& r) { return r.ema_decay != 0.f; }
inline bool clip_on(const Recipe& r) { return r.clip_max != 0.f; }
inline bool dropout_on(const Recipe& r) { return r.drop_p != 0.f; }

// The launches of a step's reduction, chosen here and nowhere else.  acc: the queued slabs go through k_reduce_all_acc<first> into the
// accumulator; update: an update launch runs, k_reduce_update<clip, plain | sgd | adam, ema, dlr> (adam: with k_adam_tick directly in front
// of it); buffered: it reads the step's gradient from a buffer (the accumulator, the clipped step's gradient buffer) as one-chunk slabs,
// behind a first launch that fills that buffer.
struct UpdateChoice { bool acc, first, update, clip, sgd, ema, dlr, buffered, adam; };
// apply false: a gradients-only walk; micro: which micro-step of an accumulating net (kWholeStep: the net does not accumulate)
inline UpdateChoice select_update(const Recipe& r, bool apply, int micro, bool lr_from_device) {
    UpdateChoice c{};
    c.acc = apply && micro != kWholeStep;
    c.first = micro == kMicroFirst;
    c.update = apply && (!c.acc || micro == kMicroLast);
    c.clip = c.update && clip_on(r);
    c.adam = c.update && adam_on(r);
    c.sgd = c.update && !c.adam && !sgd_default(r);
    c.ema = c.update && ema_on(r);
    c.dlr = c.update && lr_from_device;
    c.buffered = c.acc || c.clip;
    return c;
}

// The plan's lines for it.  An instantiation of k_reduce_update is printed as k_reduce_all[_clip][_sgd | _adam][_ema][_dlr], its display name.
// blocks: workgroups over the queued slabs; ublocks: over the one-chunk slabs of a buffered update; nblocks: of the norm over n_pad elements.
inline std::string describe_update(const UpdateChoice& c, const Recipe& r, int njobs, long long blocks, int ublocks, long long n_pad, long long nblocks) {
    std::string s;
    if (c.acc) s += strf("  reduction: k_reduce_all_acc<%s>, %d layers' slabs in one launch, %lld workgroups (accumulate: micro-batch of %d, no update)\n", c.first ? "first" : "next", njobs, blocks, r.accum_k);
    else if (c.clip) s += strf("  gradient: k_reduce_all, %d layers' slabs in one launch, %lld workgroups, into the net's gradient buffer (no update)\n", njobs, blocks);
    if (c.clip) s += strf("  norm: k_grad_sumsq, %lld elements, %lld workgroups (partial sums of squares in double, fixed order)\n", n_pad, nblocks);
    if (c.buffered && !c.update) return s;
    if (c.adam) s += "  tick: k_adam_tick, 1 thread (update count and bias corrections on the device)\n";
    s += strf("  update: k_reduce_all%s%s%s%s, ", c.clip ? "_clip" : "", c.adam ? "_adam" : c.sgd ? "_sgd" : "", c.ema ? "_ema" : "", c.dlr ? "_dlr" : "");
    s += c.buffered ? strf("%d layers' gradients as one-chunk slabs, %d workgroups", njobs, ublocks) : strf("%d layers' slabs in one launch, %lld workgroups", njobs, blocks);
    if (c.sgd) s += strf(" (SGD: momentum %g, weight decay %g, nesterov %s)", (double)r.sgd_mu, (double)r.sgd_wd, r.sgd_nesterov ? "on" : "off");
    if (c.adam) s += strf(" (Adam: betas %g %g, eps %g, weight decay %g, %s)", (double)r.adam_b1, (double)r.adam_b2, (double)r.adam_eps, (double)r.adam_wd, r.adam_decoupled ? "decoupled" : "L2");
    if (c.ema) s += strf(" (EMA: decay %g)", (double)r.ema_decay);
    if (c.clip) s += strf(" (clip: max norm %g)", (double)r.clip_max);
    if (c.acc) s += strf(" (accumulate: %d micro-batches, scale %g)", r.accum_k, (double)r.accum_c);
    return s + "\n";
}

}  // namespace rcnx
