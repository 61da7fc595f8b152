// convnet_dw_s2.hpp -- Track X: the strided depthwise 3x3 convolution (RCN_HIPX_DWCONV3X3_S2), torch.nn.Conv2d(C, C, 3, stride=2, padding=1,
// groups=C) on an even H x W map: y[b][i][j][c] = b[c] + sum_t W[t][c] x[b][2i + kh - 1][2j + kw - 1][c], t = 3 kh + kw, output oH x oW =
// (H/2) x (W/2).  18 FLOP per OUTPUT element against 4 bytes written and 16 read: streaming stencils, fp32 in either precision mode.  On an
// even map only the top row (-1) and the left column (-1) are ever outside; the bottom and the right never are.  k_dw and k_dw_wgrad
// (convnet_dw.hpp) are untouched: stride-1 nets run the instructions they ran.
//
//   k_dw_s2_fwd      A lane owns one 16-byte OUTPUT piece of a row -- output column j, channel quad cq -- and walks down a band of TH output
//                    rows.  Output row i reads input rows 2i - 1, 2i, 2i + 1, three pieces each (columns 2j - 1, 2j, 2j + 1); row 2i + 1 is
//                    row 2(i + 1) - 1 of the next output row, so per output row the lane loads TWO new input rows x three pieces and keeps
//                    one, the two new rows issued an output row ahead of their use (6 x 16 bytes in flight under the 9 pieces in use).
//                    Piece 2j + 1 is piece 2(j + 1) - 1 of the lane C/4 further on: served by the CU's L1, every input byte comes from
//                    HBM once per launch apart from one halo row per band.  A tile is (image, band of TH output rows, slab of 256 output
//                    pieces); the grid loops over the tiles.  Weights and bias of the quad (40 floats) are loaded once per workgroup where
//                    256 % (C / 4) == 0, else once per tile.  Summation order: bias, then taps 0 .. 8.
//   k_dw_s2_dgrad    The input gradient as ONE launch that writes EVERY element of dX exactly once, by one thread, with no accumulation --
//                    what launch_skip_bwd behind it (it ADDS into dX) and the bucket walk (a bucket may end behind this launch) rest on.
//                    A lane owns the 2 x 2 block of input pixels (2i .. 2i + 1, 2j .. 2j + 1) of a channel quad and walks down i over a
//                    band of TH block rows, holding two rows x two pieces of dZ -- (i, j), (i, j + 1), (i + 1, j), (i + 1, j + 1), with
//                    dZ[oH][.] = dZ[.][oW] = 0 as clamp-address / zero-value predicates -- and loading the two pieces of row i + 2 a block
//                    row ahead.  It reads W AS STORED (not the tap-flipped copy): all nine taps are used once per block, the four parity
//                    classes with 1 / 2 / 2 / 4 taps, each sum in the order written here:
//                        dX[2i][2j]         = W11 dZ[i][j]
//                        dX[2i][2j + 1]     = W10 dZ[i][j + 1] + W12 dZ[i][j]
//                        dX[2i + 1][2j]     = W01 dZ[i + 1][j] + W21 dZ[i][j]
//                        dX[2i + 1][2j + 1] = W00 dZ[i + 1][j + 1] + W02 dZ[i + 1][j] + W20 dZ[i][j + 1] + W22 dZ[i][j]
//                    H and W are even, so the blocks partition the map and the tiles (image, band, slab of 256 blocks of a block row)
//                    partition the blocks: the single write.  EPI 0: raw; EPI 3: each of the four pieces gated by G > 0, G shaped like dX
//                    (the output of the ReLU layer below).  A lane's two stores per input row are the 16-byte pieces 2j and 2j + 1 of
//                    the quad; the lanes of a wave cover 2 x C x 4-byte runs of a row between them.
//   k_dw_s2_wgrad    k_dw_wgrad's slab contract unchanged: one partial [10][C] tile (bias row last) per chunk of consecutive OUTPUT pixels
//                    m = (b oH + i) oW + j, x read at (2i + kh - 1, 2j + kw - 1), finished by the step's reduction launch in chunk order.
//                    Workgroup (chunk, 32-channel group), the in-wave xor reduction (8, 16, 32) and the in-order sum of the four waves
//                    through 5 KB of LDS are k_dw_wgrad's.
//
// 16-byte accesses, 64-bit element offsets, no atomics, no flags, no coupling between workgroups, no LDS but the weight gradient's wave
// sum, no scratch, one fixed summation order: two runs give the same bits.  (The library is built with the compiler's default contraction,
// so a `y += w * x` chain may be fused multiply-adds: the ORDER of the terms is fixed and the instructions are the same every run, which is
// what the bit-for-bit claims rest on; the roundings are not promised to be one per operation, as convnet_bn.hpp's are.)
// From the gfx950 compile (VGPRs / LDS bytes / scratch bytes; waves per SIMD): k_dw_s2_fwd 118 / 0 / 0; 4.  k_dw_s2_dgrad<0> 86 / 0 / 0; 5,
// <3> 114 / 0 / 0; 4.  k_dw_s2_wgrad 96 / 5120 / 0; 5.  All within the 128 VGPRs of four waves per SIMD, where k_dw (104) and k_dw_wgrad
// (112) stand.
#pragma once

#include "convnet_dw.hpp"

namespace rcnx {

// X: [N][H][W][C], H and W even, C % 4 == 0; Wt: [9][C]; bias: [C]; Y: [N][H/2][W/2][C].
// items = N x bands x slabs, bands = ceil(oH / TH), slabs = ceil(oW C / 4 / 256).  Any grid <= items; 256 threads.
__global__ __launch_bounds__(kThreads) void k_dw_s2_fwd(const float* __restrict__ X, const float* __restrict__ Wt, const float* __restrict__ bias, float* __restrict__ Y,
                                                        int H, int W, int C, int TH, long long items) {
    const int C4 = C >> 2, oH = H >> 1, oW = W >> 1;
    const int rowq = W * C4, orowq = oW * C4;                        // pieces per input and per output row
    const int slabs = (orowq + kDwSlab - 1) / kDwSlab, bands = (oH + TH - 1) / TH;
    const f32x4* const X4 = reinterpret_cast<const f32x4*>(X);
    f32x4* const Y4 = reinterpret_cast<f32x4*>(Y);
    const f32x4 zero = f32x4{0.f, 0.f, 0.f, 0.f};
    f32x4 wq[9], bq = zero;
    int have = -1;                                                   // the quad whose weights the lane holds
    for (long long item = blockIdx.x; item < items; item += gridDim.x) {
        const int slab = (int)(item % slabs);
        const long long rest = item / slabs;
        const int band = (int)(rest % bands);
        const long long img = rest / bands;
        const int pos = slab * kDwSlab + (int)threadIdx.x;
        const bool live = pos < orowq;
        const int q = live ? pos : orowq - 1;                        // (a lane past the row: a valid address, nothing stored)
        const int j = q / C4, cq = q - j * C4;
        if (cq != have) {
#pragma unroll
            for (int t = 0; t < 9; ++t) wq[t] = *reinterpret_cast<const f32x4*>(Wt + (long long)t * C + 4 * cq);
            bq = *reinterpret_cast<const f32x4*>(bias + 4 * cq);
            have = cq;
        }
        const bool wl = j > 0;                                       // column 2j - 1 is inside; 2j and 2j + 1 always are
        const int qm = 2 * j * C4 + cq, ql = wl ? qm - C4 : qm, qr = qm + C4;
        const int i0 = band * TH, i1 = i0 + TH < oH ? i0 + TH : oH;
        auto load = [&](int h) {                                     // input row h of the image, -1 <= h < H
            const bool in = h >= 0;                                  // the row predicate (only the top is ever outside)
            const f32x4* const p = X4 + (img * H + (in ? h : 0)) * (long long)rowq;
            DwRow r{p[ql], p[qm], p[qr]};
            if (!(in && wl)) r.l = zero;
            if (!in) { r.m = zero; r.r = zero; }
            return r;
        };
        DwRow a = load(2 * i0 - 1), b = load(2 * i0), c = load(2 * i0 + 1);
        for (int i = i0; i < i1; ++i) {
            DwRow nb = b, nc = c;
            if (i + 1 < i1) { nb = load(2 * i + 2); nc = load(2 * i + 3); }      // the next output row's two new rows, in flight under this row's arithmetic
            f32x4 y = bq;
            y += wq[0] * a.l; y += wq[1] * a.m; y += wq[2] * a.r;
            y += wq[3] * b.l; y += wq[4] * b.m; y += wq[5] * b.r;
            y += wq[6] * c.l; y += wq[7] * c.m; y += wq[8] * c.r;
            if (live) Y4[(img * oH + i) * (long long)orowq + q] = y;
            a = c; b = nb; c = nc;
        }
    }
}

// dZ: [N][H/2][W/2][C]; Wt: [9][C], W as stored; G (EPI 3): [N][H][W][C]; dX: [N][H][W][C], H and W even, C % 4 == 0.
// items = N x bands x slabs over the 2 x 2 blocks: bands = ceil(oH / TH), slabs = ceil(oW C / 4 / 256).  Any grid <= items; 256 threads.
template <int EPI>
__global__ __launch_bounds__(kThreads) void k_dw_s2_dgrad(const float* __restrict__ dZ, const float* __restrict__ Wt, const float* __restrict__ G, float* __restrict__ dX,
                                                          int H, int W, int C, int TH, long long items) {
    const int C4 = C >> 2, oH = H >> 1, oW = W >> 1;
    const int rowq = W * C4, orowq = oW * C4;
    const int slabs = (orowq + kDwSlab - 1) / kDwSlab, bands = (oH + TH - 1) / TH;
    const f32x4* const Z4 = reinterpret_cast<const f32x4*>(dZ);
    const f32x4* const G4 = reinterpret_cast<const f32x4*>(G);
    f32x4* const X4 = reinterpret_cast<f32x4*>(dX);
    const f32x4 zero = f32x4{0.f, 0.f, 0.f, 0.f};
    f32x4 wq[9];
    int have = -1;
    for (long long item = blockIdx.x; item < items; item += gridDim.x) {
        const int slab = (int)(item % slabs);
        const long long rest = item / slabs;
        const int band = (int)(rest % bands);
        const long long img = rest / bands;
        const int pos = slab * kDwSlab + (int)threadIdx.x;
        const bool live = pos < orowq;
        const int q = live ? pos : orowq - 1;
        const int j = q / C4, cq = q - j * C4;
        if (cq != have) {
#pragma unroll
            for (int t = 0; t < 9; ++t) wq[t] = *reinterpret_cast<const f32x4*>(Wt + (long long)t * C + 4 * cq);
            have = cq;
        }
        const bool wr = j + 1 < oW;                                  // dZ column j + 1 is inside
        const int qr = wr ? q + C4 : q;
        const int i0 = band * TH, i1 = i0 + TH < oH ? i0 + TH : oH;
        struct Pair2 { f32x4 m, r; };                                // dZ[i][j], dZ[i][j + 1]
        auto load = [&](int i) {                                     // dZ row i of the image, 0 <= i <= oH
            const bool in = i < oH;                                  // the row predicate (only the bottom is ever outside)
            const f32x4* const p = Z4 + (img * oH + (in ? i : oH - 1)) * (long long)orowq;
            Pair2 r{p[q], p[qr]};
            if (!in) r.m = zero;
            if (!(in && wr)) r.r = zero;
            return r;
        };
        Pair2 a = load(i0), b = load(i0 + 1);
        for (int i = i0; i < i1; ++i) {
            Pair2 c = b;
            if (i + 1 < i1) c = load(i + 2);                         // the row after next, in flight under this block row's arithmetic
            const long long o0 = (img * H + 2 * i) * (long long)rowq + 2 * j * C4 + cq, o1 = o0 + rowq;     // pieces (2i, 2j) and (2i + 1, 2j)
            f32x4 g00 = zero, g01 = zero, g10 = zero, g11 = zero;
            if (EPI == 3) { g00 = G4[o0]; g01 = G4[o0 + C4]; g10 = G4[o1]; g11 = G4[o1 + C4]; }
            f32x4 x00 = wq[4] * a.m;
            f32x4 x01 = wq[3] * a.r; x01 += wq[5] * a.m;
            f32x4 x10 = wq[1] * b.m; x10 += wq[7] * a.m;
            f32x4 x11 = wq[0] * b.r; x11 += wq[2] * b.m; x11 += wq[6] * a.r; x11 += wq[8] * a.m;
            if (EPI == 3) { x00 = dw_gate(x00, g00); x01 = dw_gate(x01, g01); x10 = dw_gate(x10, g10); x11 = dw_gate(x11, g11); }
            if (live) { X4[o0] = x00; X4[o0 + C4] = x01; X4[o1] = x10; X4[o1 + C4] = x11; }
            a = b; b = c;
        }
    }
}

// X: [N][H][W][C], dZ: [N][H/2][W/2][C], C % 32 == 0, M = N oH oW OUTPUT pixels; slab: [chunks][10][C].  grid (chunks, C / 32), 256 threads.
__global__ __launch_bounds__(kThreads) void k_dw_s2_wgrad(const float* __restrict__ X, const float* __restrict__ dZ, float* __restrict__ slab, long long M, int H, int W, int C,
                                                          int pix_per_chunk) {
    __shared__ f32x4 part[kThreads / 64][10][kDwGroup / 4];
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
    const int cq = tid & (kDwGroup / 4 - 1), pl = tid / (kDwGroup / 4);      // (within a wave: quad = lane & 7, pixel lane = lane >> 3)
    const int c0 = blockIdx.y * kDwGroup + 4 * cq;
    const int oH = H >> 1, oW = W >> 1;
    const long long p0 = (long long)blockIdx.x * pix_per_chunk;
    const long long p1 = p0 + pix_per_chunk < M ? p0 + pix_per_chunk : M;
    const f32x4 zero = f32x4{0.f, 0.f, 0.f, 0.f};
    f32x4 acc[10];
#pragma unroll
    for (int t = 0; t < 10; ++t) acc[t] = zero;
    for (long long m = p0 + pl; m < p1; m += kDwPixLanes) {
        const int j = (int)(m % oW);
        const long long r = m / oW;
        const int i = (int)(r % oH);
        const long long xm = ((r / oH) * H + 2 * i) * (long long)W + 2 * j;      // the input pixel (2i, 2j) under the centre tap
        const f32x4 dz = *reinterpret_cast<const f32x4*>(dZ + m * C + c0);
        f32x4 x[9];
#pragma unroll
        for (int t = 0; t < 9; ++t) {
            const int dh = t / 3 - 1, dw = t % 3 - 1;
            const bool in = 2 * i + dh >= 0 && 2 * j + dw >= 0;                  // (2i + 1 < H and 2j + 1 < W always)
            const long long mm = in ? xm + (long long)dh * W + dw : xm;          // clamp the address, zero the value
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
            for (int k = 0; k < 4; ++k) acc[t][k] += __shfl_xor(acc[t][k], off, 64);
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
