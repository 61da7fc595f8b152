// convnet_dw.hpp -- Track X: the depthwise 3x3 convolution (RCN_HIPX_DWCONV3X3), the first convolution here that is not a GEMM.
//
// On an NHWC map y[b][h][w][c] = sum_t W[t][c] x[b][h + kh - 1][w + kw - 1][c] + b[c], t = 3 kh + kw: 18 FLOP per output element against
// 8 bytes of compulsory traffic -- a streaming stencil, fp32 in either precision mode (no GEMM, so no GEMM operand to round).
//
//   k_dw<EPI>    forward (EPI 1: + bias) and input gradient (EPI 0 raw, 3 gated by G > 0; `bias` = G, shaped like Y) -- the same stencil
//                over dZ on the tap-reversed copy [8 - t][c] that k_flip_weights(3, 1, C) and FlipSpec{wt, 9, 1, C} keep current.
//                A lane owns one 16-byte piece of a map row -- pixel w, channel quad cq -- and walks down a band of TH rows with a window
//                of three rows x three pieces in registers: per output piece it issues the three loads of row h + 2 (left, own, right;
//                the left and right pieces are what the neighbouring lanes load as their own, so they are served by the CU's L1 and every
//                byte comes from HBM once per launch -- apart from the two halo rows of a band, and a whole-height band has none).  A
//                wave's loads are 1 KiB contiguous (pieces of one row are consecutive lanes).  The row after next is in flight while a row
//                is computed: 3 x 16 bytes per lane ahead of the 9 pieces in use.  Weights and bias of the quad (40 floats) are loaded once
//                per workgroup where 256 % (C / 4) == 0 (the quad then is tid % (C / 4) in every tile), else once per tile; never per pixel.
//                Borders are predicates: the address is clamped into the map and the value zeroed.  64-bit element offsets.
//                A tile is (image, band of TH rows, slab of 256 pieces of a row); the tiles partition the map, a live lane stores each
//                of its TH pieces once, so every element of Y is written exactly once, by one thread, in one fixed summation order
//                (bias, then taps 0 .. 8).  The grid loops over tiles: workgroup b takes tiles b, b + gridDim.x, ...
//   k_dw_wgrad   dW[t][c] = sum_m x[m + tap t][c] dZ[m][c], db[c] = sum_m dZ[m][c]: ten sums per channel over a chunk of consecutive
//                pixels m = (b H + h) W + w, as one partial [10][C] tile (bias row last) per chunk in the layer's slab, which the step's
//                reduction launch sums in chunk order.  Workgroup (chunk, 32-channel group): 8 channel quads x 32 pixel lanes; a lane
//                sums pixels p0 + pl, + 32, ... ascending, then the 8 pixel lanes of a wave by three xor shuffles (8, 16, 32), then the
//                four waves in order through 5 KB of LDS.  No atomics, one fixed order: two runs give the same bits.  Taps read across
//                chunk, row and image edges by the same clamp-and-zero predicates.
//
// No coupling between workgroups (no flags, no atomics), no scratch.
#pragma once

#include "convnet.hpp"

namespace rcnx {

constexpr int kDwSlab = kThreads;            // 16-byte pieces of a map row per tile (one per lane)
constexpr int kDwGroup = 32;                 // k_dw_wgrad: channels per workgroup (8 quads)
constexpr int kDwPixLanes = kThreads / (kDwGroup / 4);      // ... and its pixel lanes (32)

struct DwRow { f32x4 l, m, r; };             // three neighbouring pieces of one map row: pixels w - 1, w, w + 1 of a channel quad

__device__ inline f32x4 dw_gate(const f32x4& y, const f32x4& g) {
    return f32x4{g[0] > 0.f ? y[0] : 0.f, g[1] > 0.f ? y[1] : 0.f, g[2] > 0.f ? y[2] : 0.f, g[3] > 0.f ? y[3] : 0.f};
}

// X, Y (and G = `bias` for EPI 3): [N][H][W][C], C % 4 == 0; Wt: [9][C] (forward: W; input gradient: the tap-reversed copy); EPI 1: bias[C].
// items = N x bands x slabs, bands = ceil(H / TH), slabs = ceil(W C / 4 / 256).  Any grid <= items; 256 threads.
template <int EPI>
__global__ __launch_bounds__(kThreads) void k_dw(const float* __restrict__ X, const float* __restrict__ Wt, const float* __restrict__ bias, float* __restrict__ Y,
                                                 int H, int W, int C, int TH, long long items) {
    const int C4 = C >> 2;
    const int rowq = W * C4;                                         // pieces per map row
    const int slabs = (rowq + kDwSlab - 1) / kDwSlab, bands = (H + TH - 1) / TH;
    const f32x4* const X4 = reinterpret_cast<const f32x4*>(X);
    const f32x4* const G4 = reinterpret_cast<const f32x4*>(bias);
    f32x4* const Y4 = reinterpret_cast<f32x4*>(Y);
    const f32x4 zero = f32x4{0.f, 0.f, 0.f, 0.f};
    f32x4 wq[9], bq = zero;
    int have = -1;                                                   // the quad whose weights the lane holds
    for (long long item = blockIdx.x; item < items; item += gridDim.x) {
        const int slab = (int)(item % slabs);
        const long long rest = item / slabs;
        const int band = (int)(rest % bands);
        const long long img_row = (rest / bands) * H;                // first map row of the image, in rows of the whole tensor
        const int pos = slab * kDwSlab + (int)threadIdx.x;
        const bool live = pos < rowq;
        const int q = live ? pos : rowq - 1;                         // (a lane past the row: a valid address, nothing stored)
        const int w = q / C4, cq = q - w * C4;
        if (cq != have) {
#pragma unroll
            for (int t = 0; t < 9; ++t) wq[t] = *reinterpret_cast<const f32x4*>(Wt + (long long)t * C + 4 * cq);
            if (EPI == 1) bq = *reinterpret_cast<const f32x4*>(bias + 4 * cq);
            have = cq;
        }
        const bool wl = w > 0, wr = w + 1 < W;
        const int ql = wl ? q - C4 : q, qr = wr ? q + C4 : q;        // the column predicates, as address clamps
        const int h0 = band * TH, h1 = h0 + TH < H ? h0 + TH : H;
        auto load = [&](int h) {
            const bool in = h >= 0 && h < H;                         // the row predicate
            const int hc = h < 0 ? 0 : h < H ? h : H - 1;
            const f32x4* const p = X4 + (img_row + hc) * (long long)rowq;
            DwRow r{p[ql], p[q], p[qr]};
            if (!(in && wl)) r.l = zero;
            if (!in) r.m = zero;
            if (!(in && wr)) r.r = zero;
            return r;
        };
        DwRow a = load(h0 - 1), b = load(h0), c = load(h0 + 1);
        for (int h = h0; h < h1; ++h) {
            DwRow d = c;
            if (h + 1 < h1) d = load(h + 2);                         // the row after next, in flight under this row's arithmetic
            const long long o = (img_row + h) * (long long)rowq + q;
            f32x4 g = zero;
            if (EPI == 3) g = G4[o];
            f32x4 y = bq;
            y += wq[0] * a.l; y += wq[1] * a.m; y += wq[2] * a.r;
            y += wq[3] * b.l; y += wq[4] * b.m; y += wq[5] * b.r;
            y += wq[6] * c.l; y += wq[7] * c.m; y += wq[8] * c.r;
            if (EPI == 3) y = dw_gate(y, g);
            if (live) Y4[o] = y;
            a = b; b = c; c = d;
        }
    }
}

// X, dZ: [N][H][W][C], C % 32 == 0, M = N H W pixels; slab: [chunks][10][C].  grid (chunks, C / 32), 256 threads.
__global__ __launch_bounds__(kThreads) void k_dw_wgrad(const float* __restrict__ X, const float* __restrict__ dZ, float* __restrict__ slab, long long M, int H, int W, int C,
                                                       int pix_per_chunk) {
    __shared__ f32x4 part[kThreads / 64][10][kDwGroup / 4];
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
    const int cq = tid & (kDwGroup / 4 - 1), pl = tid / (kDwGroup / 4);      // (within a wave: quad = lane & 7, pixel lane = lane >> 3)
    const int c0 = blockIdx.y * kDwGroup + 4 * cq;
    const long long p0 = (long long)blockIdx.x * pix_per_chunk;
    const long long p1 = p0 + pix_per_chunk < M ? p0 + pix_per_chunk : M;
    const f32x4 zero = f32x4{0.f, 0.f, 0.f, 0.f};
    f32x4 acc[10];
#pragma unroll
    for (int t = 0; t < 10; ++t) acc[t] = zero;
    for (long long m = p0 + pl; m < p1; m += kDwPixLanes) {
        const int w = (int)(m % W);
        const int h = (int)((m / W) % H);
        const f32x4 dz = *reinterpret_cast<const f32x4*>(dZ + m * C + c0);
        f32x4 x[9];
#pragma unroll
        for (int t = 0; t < 9; ++t) {
            const int dh = t / 3 - 1, dw = t % 3 - 1;
            const bool in = h + dh >= 0 && h + dh < H && w + dw >= 0 && w + dw < W;
            const long long mm = in ? m + (long long)dh * W + dw : m;          // clamp the address, zero the value
            const f32x4 v = *reinterpret_cast<const f32x4*>(X + mm * C + c0);
            x[t] = in ? v : zero;
        }
#pragma unroll
        for (int t = 0; t < 9; ++t) acc[t] += x[t] * dz;
        acc[9] += dz;
    }
    // the eight pixel lanes of a wave, in one fixed order
#pragma unroll
    for (int t = 0; t < 10; ++t)
#pragma unroll
        for (int off = 8; off < 64; off <<= 1)
#pragma unroll
            for (int j = 0; j < 4; ++j) acc[t][j] += __shfl_xor(acc[t][j], off, 64);
    if (lane < kDwGroup / 4) {
#pragma unroll
        for (int t = 0; t < 10; ++t) part[wave][t][lane] = acc[t];
    }
    __syncthreads();
    // ... and the four waves, in order: 80 pieces of the [10][32] tile
    if (tid < 10 * (kDwGroup / 4)) {
        const int t = tid / (kDwGroup / 4), qd = tid - t * (kDwGroup / 4);
        f32x4 s = part[0][t][qd];
#pragma unroll
        for (int v = 1; v < kThreads / 64; ++v) s += part[v][t][qd];
        *reinterpret_cast<f32x4*>(slab + ((long long)blockIdx.x * 10 + t) * C + blockIdx.y * kDwGroup + 4 * qd) = s;
    }
}

}  // namespace rcnx
