// convnet_halo_bf16.hpp -- Track X, bf16 MFMA path: the LDS-tiled 3x3 kernels.  No reference counterpart.
//
//   k_conv3x3_halo_bf16      forward / input gradient, one work item per workgroup, operands staged in place
//   k_wgrad3x3_halo_bf16     weight gradient: nine waves = nine filter taps over one staged halo + dZ block
//   k_conv3x3_halo_bf16p     forward / input gradient as a software pipeline (round 3)
//   k_conv3x3_halo_bf16_1cb  the same for layers of exactly 32 input channels: the weights stay in LDS
//
// k_conv3x3_halo_bf16 has the right data flow -- one staged halo per 8 x 16 pixel block serves all nine taps --
// but loads, waits, converts and stores every operand in place, with two barriers per filter row and one work item per workgroup:
// on the 224 x 224 net it ran at 15 % of the bf16 MFMA rate AND 4.7 x its HBM floor, i.e. on latency and integer instructions.
// k_conv3x3_halo_bf16p is the same kernel on the frame round 3 built for the fp32 path (convnet_halo.hpp): work items walked by a
// resident grid (ItemWalk), phases (item, channel block, filter row) whose operands are loaded into registers one phase ahead of their
// use -- across item boundaries too --, every thread's share of the staged grids decoded once (StageMap), the epilogues
// shared (halo_epilogue).  Same LDS images, same operand rounding (RNE to bf16 on the way into LDS, fp32 accumulation), same MFMA order
// as k_conv3x3_halo_bf16: bit-identical results.
#pragma once

#include "convnet_bf16.hpp"
#include "convnet_halo.hpp"

namespace rcnx {

// ---------------------------------------------------------------------------------------------------------------------
// k_conv3x3_halo_bf16 -- 3x3 convolution, LDS-tiled (channel blocks of 32 or 64).
//
// The implicit-GEMM kernel (convnet_bf16.hpp) re-reads every input pixel once per filter tap (nine shifted A tiles out of L2); for
// thin layers that traffic, not the MFMA, is the limit (5-7 % MFMA-busy by PMC at Cin = 32).  Here a workgroup owns an
// 8 x 16 block of output pixels of one image and stages the 10 x 18 input HALO of one channel block, as bf16, in LDS; all nine
// taps then read their A fragments out of that one image (a lane's eight consecutive channels of pixel (y + kh, x + kw):
// one ds_read_b128, no im2col anywhere), so global A traffic drops from 9 x 128 to 180 pixel rows per tile.  The bf16
// weights of one filter row (3 taps x BN x Cin) sit beside it and are restaged per filter row.  Wave w computes output
// rows 2w, 2w+1 of the block (32 pixels) x BN channels.  Same operands, rounding and epilogues as k_conv_fwd_bf16, so
// the two are interchangeable; used for forward and (on dZ with the flipped weights) for the input gradient.
template <int CB, int BN, int EPI, bool PIN = false>
__global__ __launch_bounds__(kThreads) void k_conv3x3_halo_bf16(const float* __restrict__ X, const __bf16* __restrict__ WB,
                                                                const float* __restrict__ bias, float* __restrict__ Y, ConvShape s, int tiles_w,
                                                                int tiles_h, uint8_t* __restrict__ pool_idx, PooledGrad pin) {
    static_assert(CB % 16 == 0 && BN % 32 == 0, "channel blocks of the 32x32x16 MFMA");
    constexpr int NT = BN / 32, LDC = CB + 8;                        // halves per pixel / per weight row in LDS (16-byte aligned, bank-skewed)
    constexpr int HH = kHaloTH + 2, HW = kHaloTW + 2;
    constexpr int HCH = HH * HW * (CB / 4);                           // f32x4 chunks of one channel block of the halo
    constexpr int BCH = 3 * BN * (CB / 8);                            // 16-byte chunks of one filter row's weights for that block
    __shared__ __attribute__((aligned(16))) __bf16 Hs[HH * HW * LDC];
    __shared__ __attribute__((aligned(16))) __bf16 Bs[3 * BN * LDC];
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
    int tile = blockIdx.x;
    const int tw = tile % tiles_w; tile /= tiles_w;
    const int th = tile % tiles_h;
    const int img = tile / tiles_h;
    const int oh0 = th * kHaloTH, ow0 = tw * kHaloTW, n0 = blockIdx.y * BN;
    const int Cin = s.Cin, K = 9 * Cin;                               // Cin: a multiple of CB; K = row length of WB

    f32x16 acc[NT];
#pragma unroll
    for (int t = 0; t < NT; ++t)
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[t][r] = 0.f;
    const int r = lane & 31, h = lane >> 5;
    const int py = 2 * wave + (r >> 4), px = r & 15;                  // this lane's A row = output pixel (py, px) of the block
#pragma unroll 1
    for (int cb = 0; cb < Cin; cb += CB) {
        if (cb) __syncthreads();                                      // the previous channel block's halo has been consumed
        // ---- halo: pixel (oh0 - 1 + hy, ow0 - 1 + hx), channels cb .. cb + CB - 1, zero outside the image; unconditional
        // loads from clamped addresses
        if (PIN) {
            // the input is a pooled-resolution gradient: one thread loads (dP, P, arg-max) of ONE pooled pixel's four channels -- the 6 x 10
            // pooled pixels under the halo -- and expands it into the up to four halo pixels of its window (round 3: a load triple per
            // halo pixel had fetched every pooled value four times; these kernels were 1.6 x their forward twins)
            constexpr int PPW = kHaloTW / 2 + 2, PCH = 6 * PPW * (CB / 4);
            for (int e = tid; e < PCH; e += kThreads) {
                const int pp = e / (CB / 4), c4 = (e - pp * (CB / 4)) * 4;
                const int pr = pp / PPW, pc = pp - pr * PPW;
                const int poh = (oh0 >> 1) - 1 + pr, pow_ = (ow0 >> 1) - 1 + pc;
                const bool ok = (unsigned)poh < (unsigned)(s.H >> 1) && (unsigned)pow_ < (unsigned)(s.W >> 1);
                const long long o = ok ? (((long long)img * (s.H >> 1) + poh) * (s.W >> 1) + pow_) * Cin + cb + c4 : 0;
                const f32x4 d = *reinterpret_cast<const f32x4*>(pin.dP + o), pv = *reinterpret_cast<const f32x4*>(pin.P + o);
                const unsigned ii = *reinterpret_cast<const unsigned*>(pin.idx + o);
                f32x4 v[4];
                unpool4x4(ok ? d : f32x4{0, 0, 0, 0}, pv, ii, v);
#pragma unroll
                for (int pos = 0; pos < 4; ++pos) {
                    const int hy = 2 * pr - 1 + (pos >> 1), hx = 2 * pc - 1 + (pos & 1);
                    if ((unsigned)hy < (unsigned)HH && (unsigned)hx < (unsigned)HW)
                        *reinterpret_cast<bf16x4*>(&Hs[(hy * HW + hx) * LDC + c4]) = to_bf16x4(v[pos]);
                }
            }
        } else {
            for (int e = tid; e < HCH; e += kThreads) {
                const int pix = e / (CB / 4), c4 = (e - pix * (CB / 4)) * 4;
                const int hy = pix / HW, hx = pix - hy * HW;
                const int ih = oh0 - 1 + hy, iw = ow0 - 1 + hx;
                const bool ok = (unsigned)ih < (unsigned)s.H && (unsigned)iw < (unsigned)s.W;
                const f32x4 v = *reinterpret_cast<const f32x4*>(X + (ok ? (((long long)img * s.H + ih) * s.W + iw) * Cin + cb + c4 : 0));
                *reinterpret_cast<bf16x4*>(&Hs[pix * LDC + c4]) = to_bf16x4(ok ? v : f32x4{0, 0, 0, 0});
            }
        }
#pragma unroll 1
        for (int kh = 0; kh < 3; ++kh) {
            if (kh) __syncthreads();                                  // everyone is done with the previous filter row's weights
            for (int e = tid; e < BCH; e += kThreads) {
                const int row = e / (CB / 8), c8 = (e - row * (CB / 8)) * 8;    // row = kw * BN + co
                const int kw = row / BN, co = row - kw * BN;
                *reinterpret_cast<bf16x8*>(&Bs[row * LDC + c8]) =
                    *reinterpret_cast<const bf16x8*>(WB + (long long)(n0 + co) * K + (kh * 3 + kw) * Cin + cb + c8);
            }
            __syncthreads();
#pragma unroll
            for (int kw = 0; kw < 3; ++kw) {
                const __bf16* a = &Hs[((py + kh) * HW + px + kw) * LDC + 8 * h];
                const __bf16* b = &Bs[(kw * BN + r) * LDC + 8 * h];
#pragma unroll
                for (int ks = 0; ks < CB / 16; ++ks) {
                    const bf16x8 af = *reinterpret_cast<const bf16x8*>(a + 16 * ks);
#pragma unroll
                    for (int t = 0; t < NT; ++t) {
                        const bf16x8 bf = *reinterpret_cast<const bf16x8*>(b + 32 * t * LDC + 16 * ks);
                        acc[t] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(af, bf, acc[t], 0, 0, 0);
                    }
                }
            }
        }
    }
    // ---- epilogue: accumulator row i of lane = block pixel mfma32_row(lane, i) of this wave's 32
    if (EPI == 4) {
        // bias + ReLU + the 2x2 max-pool that follows, fused: a lane's sixteen rows are columns 4h..4h+3 and 8+4h..8+4h+3 of BOTH
        // pixel rows of its wave, i.e. four complete pooling windows -- the pool is a max over the lane's own registers.  Writes the
        // pooled map and the arg-max image exactly as k_pool_fwd does (first maximum in the order 00, 01, 10, 11), so k_pool_bwd is
        // unchanged; the un-pooled activation is never written.
        const int OH = s.H / 2, OW = s.W / 2;
        const int poh = oh0 / 2 + wave;
#pragma unroll
        for (int t = 0; t < NT; ++t) {
            const int co = n0 + 32 * t + (lane & 31);
            const float bb = bias[co];
#pragma unroll
            for (int gq = 0; gq < 2; ++gq)
#pragma unroll
                for (int pp = 0; pp < 2; ++pp) {
                    const int i0 = 4 * gq + 2 * pp;
                    float v[4] = {acc[t][i0] + bb, acc[t][i0 + 1] + bb, acc[t][8 + i0] + bb, acc[t][8 + i0 + 1] + bb};
#pragma unroll
                    for (int k = 0; k < 4; ++k) v[k] = v[k] > 0.f ? v[k] : 0.f;
                    float best = v[0];
                    int bk = 0;
#pragma unroll
                    for (int k = 1; k < 4; ++k)
                        if (v[k] > best) { best = v[k]; bk = k; }
                    const int pow_ = ow0 / 2 + 2 * h + 4 * gq + pp;
                    const bool ok = poh < OH && pow_ < OW;
                    const long long o = (((long long)img * OH + poh) * OW + pow_) * s.Cout + co;
                    if (ok) Y[o] = best;
                    store_idx_quad(pool_idx, o, bk, ok, lane);
                }
        }
        return;
    }
#pragma unroll
    for (int t = 0; t < NT; ++t) {
        const int co = n0 + 32 * t + (lane & 31);
        const float bb = (EPI == 1 || EPI == 2) ? bias[co] : 0.f;
#pragma unroll
        for (int i = 0; i < 16; ++i) {
            const int pr = mfma32_row(lane, i);
            const int oh = oh0 + 2 * wave + (pr >> 4), ow = ow0 + (pr & 15);
            if (oh < s.H && ow < s.W) {
                const long long m = ((long long)img * s.H + oh) * s.W + ow;
                float v = acc[t][i] + bb;
                if (EPI == 2) v = v > 0.f ? v : 0.f;
                if (EPI == 3) v = bias[m * s.Cout + co] > 0.f ? v : 0.f;
                Y[m * s.Cout + co] = v;
            }
        }
    }
}

// ---------------------------------------------------------------------------------------------------------------------
// k_wgrad3x3_halo_bf16 -- weight gradient of a 3x3 layer, LDS-tiled: the companion of k_conv3x3_halo_bf16.
//
// k_conv_wgrad_bf16 gives every 32-row k-block (= one filter tap of 32 channels) its own staged X tile, i.e. reads the
// input nine times and dZ once per k-group.  Here a workgroup stages, per 8 x 16 block of output pixels, the 10 x 18 input
// halo of one channel block and the block's dZ ONCE, and its NINE waves each contract one filter tap over the block:
// wave (kh, kw) reads its A fragments -- 16 consecutive pixels of halo row py + kh starting at column kw, 32 channels -- and
// the shared dZ fragments with the hardware transposed LDS read (the contraction index, the pixel, is the row of both LDS
// images), accumulating dW[tap][ci][co] in registers across all the blocks of its chunk.  Global traffic per block: 180
// input pixels + 128 dZ pixels instead of 9 x 128 + 128 per k-group.  Output: the same slab[chunk][K + 1][Cout] as
// k_conv_wgrad (row K = bias partial, fp32 sums of the unrounded dZ), so the reduction launch finishes either.
constexpr int kWgHaloThreads = 9 * 64;

// TS: storage type of X, dZ and the pooled gradient (convnet.hpp, Chunk4)
template <int CB, int BN, bool PDZ = false, typename TS = float>
__global__ __launch_bounds__(kWgHaloThreads) void k_wgrad3x3_halo_bf16(const TS* __restrict__ X, const TS* __restrict__ dZ,
                                                                       float* __restrict__ slab, ConvShape s, int tiles_w, int tiles_h,
                                                                       int blocks_per_chunk, int n_chunks, PooledGradT<TS> pdz) {
    constexpr int NA = CB / 32, NT = BN / 32, LDC = CB + 8, LDD = BN + 8;
    constexpr int HH = kHaloTH + 2, HW = kHaloTW + 2, NPX = kHaloTH * kHaloTW;
    constexpr int HCH = HH * HW * (CB / 4), DCH = NPX * (BN / 4);
    __shared__ __attribute__((aligned(16))) __bf16 Hs[HH * HW * LDC];
    __shared__ __attribute__((aligned(16))) __bf16 Ds[NPX * LDD];
    __shared__ __attribute__((aligned(16))) float red[kWgHaloThreads * 4];
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
    const int kh = wave / 3, kw = wave - 3 * kh;                      // this wave's filter tap
    const int cb = blockIdx.x * CB, n0 = blockIdx.y * BN, chunk = blockIdx.z;
    const int Cin = s.Cin, K = 9 * Cin;
    const int total_blocks = tiles_w * tiles_h * s.N;
    const int b0 = chunk * blocks_per_chunk, b1 = b0 + blocks_per_chunk < total_blocks ? b0 + blocks_per_chunk : total_blocks;

    f32x16 acc[NA][NT];
#pragma unroll
    for (int g = 0; g < NA; ++g)
#pragma unroll
        for (int t = 0; t < NT; ++t)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[g][t][r] = 0.f;
    f32x4 colsum = {0.f, 0.f, 0.f, 0.f};

    // Staging in two steps (round 3): the global loads of block blk + 1 are issued into registers before block blk is contracted and
    // stored to LDS after it -- with one 576-thread workgroup per CU (64 accumulator registers per wave) nothing else covered their
    // latency.  A thread's chunks: halo chunk q = 4 channels of halo pixel (tid + 576 q) / (CB/4); dZ chunk q likewise over the block's
    // 128 pixels, or, PDZ, ONE pooled pixel's (dP, P, arg-max), expanded into its window when stored.
    constexpr int NHQ = (HCH + kWgHaloThreads - 1) / kWgHaloThreads, NDQ = PDZ ? 1 : (DCH + kWgHaloThreads - 1) / kWgHaloThreads;
    static_assert(!PDZ || 32 * (BN / 4) <= kWgHaloThreads, "one pooled chunk per thread");
    int hrel[NHQ];                                                    // (hy * W + hx) * Cin + c4, or -1: no such chunk; hy | hx << 8 in hpk
    int hpk[NHQ];
#pragma unroll
    for (int q = 0; q < NHQ; ++q) {
        const int e = tid + kWgHaloThreads * q;
        const int pix = e / (CB / 4), c4 = (e - pix * (CB / 4)) * 4;
        const int hy = pix / HW, hx = pix - hy * HW;
        hpk[q] = e < HCH ? (hy | (hx << 8)) : -1;
        hrel[q] = (hy * s.W + hx) * Cin + c4;
    }
    // S blocks' operands are in flight at once (round 4; one was: a 32-channel layer's block is 8 MFMAs per wave against a load latency
    // of more than a microsecond, with ONE workgroup per CU -- the kernel ran at exactly blocks x latency).  A stage is a handful of
    // registers, refilled with the block S further on as soon as its own block has gone to LDS; every gload issues the same number of
    // loads whatever the block (past the chunk's last block: that block again), so the wait in front of a stage's LDS stores is an exact
    // count that leaves the younger stages in flight.  (64 x 64 tiles: 64 accumulator registers, and a block is 32 MFMAs per wave; fp32
    // tensors: twice the registers per stage.)
    constexpr int S = sizeof(TS) == 4 ? (NA * NT == 4 ? 1 : 2) : (NA * NT == 1 ? 4 : NA * NT == 2 ? 3 : PDZ ? 2 : 1);
    struct Stage { chunk4_t<TS> hv[NHQ], dv[NDQ], dpv; unsigned dii, okm; };
    Stage stg[S];
    auto gload = [&](int blk, Stage& g) {
        chunk4_t<TS> (&hv)[NHQ] = g.hv; chunk4_t<TS> (&dv)[NDQ] = g.dv; chunk4_t<TS>& dpv = g.dpv; unsigned& dii = g.dii; unsigned& okm = g.okm;
        int q0 = blk;
        const int tw = q0 % tiles_w; q0 /= tiles_w;
        const int th = q0 % tiles_h;
        const int img = q0 / tiles_h;
        const int oh0 = th * kHaloTH, ow0 = tw * kHaloTW;
        const long long hbase = (((long long)img * s.H + oh0 - 1) * s.W + ow0 - 1) * Cin + cb;
        okm = 0;
#pragma unroll
        for (int q = 0; q < NHQ; ++q) {
            const int pk = hpk[q];
            const bool ok = pk >= 0 && (unsigned)(oh0 - 1 + (pk & 255)) < (unsigned)s.H && (unsigned)(ow0 - 1 + (pk >> 8)) < (unsigned)s.W;
            okm |= (ok ? 1u : 0u) << q;
            hv[q] = *reinterpret_cast<const chunk4_t<TS>*>(X + (ok ? hbase + hrel[q] : 0));
        }
        if (PDZ) {
            const int pp = tid / (BN / 4), c4 = (tid - pp * (BN / 4)) * 4;
            const int poh = (oh0 >> 1) + (pp >> 3), pow_ = (ow0 >> 1) + (pp & 7);
            const bool ok = tid < 32 * (BN / 4) && poh < (s.H >> 1) && pow_ < (s.W >> 1);
            okm |= (ok ? 1u : 0u) << 16;
            const long long o = ok ? (((long long)img * (s.H >> 1) + poh) * (s.W >> 1) + pow_) * s.Cout + n0 + c4 : 0;
            dv[0] = *reinterpret_cast<const chunk4_t<TS>*>(pdz.dP + o);
            dpv = *reinterpret_cast<const chunk4_t<TS>*>(pdz.P + o);
            dii = *reinterpret_cast<const unsigned*>(pdz.idx + o);
        } else {
#pragma unroll
            for (int q = 0; q < NDQ; ++q) {
                const int e = tid + kWgHaloThreads * q;
                const int pix = e / (BN / 4), c4 = (e - pix * (BN / 4)) * 4;
                const int oh = oh0 + pix / kHaloTW, ow = ow0 + pix % kHaloTW;
                const bool ok = e < DCH && oh < s.H && ow < s.W;
                okm |= (ok ? 1u : 0u) << (16 + q);
                dv[q] = *reinterpret_cast<const chunk4_t<TS>*>(dZ + (ok ? (((long long)img * s.H + oh) * s.W + ow) * s.Cout + n0 + c4 : 0));
            }
        }
    };
    auto lstore = [&](const Stage& g) {
        const chunk4_t<TS> (&hv)[NHQ] = g.hv; const chunk4_t<TS> (&dv)[NDQ] = g.dv; const chunk4_t<TS>& dpv = g.dpv; const unsigned dii = g.dii, okm = g.okm;
#pragma unroll
        for (int q = 0; q < NHQ; ++q) {
            const int e = tid + kWgHaloThreads * q;
            const int pix = e / (CB / 4), c4 = (e - pix * (CB / 4)) * 4;
            if (NHQ * kWgHaloThreads == HCH || e < HCH) *reinterpret_cast<bf16x4*>(&Hs[pix * LDC + c4]) = ((okm >> q) & 1u) ? to_bf16x4(hv[q]) : bf16x4{(__bf16)0.f, (__bf16)0.f, (__bf16)0.f, (__bf16)0.f};
        }
        if (PDZ) {
            if (tid < 32 * (BN / 4)) {
                const int pp = tid / (BN / 4), c4 = (tid - pp * (BN / 4)) * 4;
                const int ppy = pp >> 3, ppx = pp & 7;
                f32x4 v[4];
                unpool4x4(((okm >> 16) & 1u) ? widen4(dv[0]) : f32x4{0, 0, 0, 0}, widen4(dpv), dii, v);
#pragma unroll
                for (int pos = 0; pos < 4; ++pos) {
                    *reinterpret_cast<bf16x4*>(&Ds[((2 * ppy + (pos >> 1)) * kHaloTW + 2 * ppx + (pos & 1)) * LDD + c4]) = to_bf16x4(v[pos]);
                    colsum += v[pos];                                 // fp32, unrounded: the bias gradient (a thread's columns are the same for every block)
                }
            }
        } else {
#pragma unroll
            for (int q = 0; q < NDQ; ++q) {
                const int e = tid + kWgHaloThreads * q;
                const int pix = e / (BN / 4), c4 = (e - pix * (BN / 4)) * 4;
                if (NDQ * kWgHaloThreads == DCH || e < DCH) {
                    const f32x4 v = ((okm >> (16 + q)) & 1u) ? widen4(dv[q]) : f32x4{0, 0, 0, 0};
                    *reinterpret_cast<bf16x4*>(&Ds[pix * LDD + c4]) = to_bf16x4(v);
                    colsum += v;                                      // fp32, unrounded: the bias gradient (same columns every time: 576 % (BN/4) == 0)
                }
            }
        }
    };

    if (b0 < b1) {
#pragma unroll
        for (int u = 0; u < S; ++u) gload(b0 + u < b1 ? b0 + u : b1 - 1, stg[u]);
    }
#pragma unroll 1
    for (int blk0 = b0; blk0 < b1; blk0 += S)
#pragma unroll
    for (int u = 0; u < S; ++u) {
        const int blk = blk0 + u;
        if (blk >= b1) break;
        if (blk != b0) __syncthreads();                               // the previous block's images have been consumed
        lstore(stg[u]);
        __syncthreads();
        gload(blk + S < b1 ? blk + S : b1 - 1, stg[u]);              // S blocks ahead, under this and the next blocks' MFMAs
#pragma unroll
        for (int py = 0; py < kHaloTH; ++py) {                        // one 16-pixel contraction step per block row
            bf16x8 af[NA], bf[NT];
#pragma unroll
            for (int a = 0; a < NA; ++a) af[a] = tr_fragment(Hs + ((py + kh) * HW + kw) * LDC, LDC, 0, 32 * a, lane);
#pragma unroll
            for (int t = 0; t < NT; ++t) bf[t] = tr_fragment(Ds + py * kHaloTW * LDD, LDD, 0, 32 * t, lane);
#pragma unroll
            for (int a = 0; a < NA; ++a)
#pragma unroll
                for (int t = 0; t < NT; ++t) acc[a][t] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(af[a], bf[t], acc[a][t], 0, 0, 0);
        }
    }
    float* out = slab + (long long)chunk * (K + 1) * s.Cout;
    const int krow0 = (kh * 3 + kw) * Cin + cb;
#pragma unroll
    for (int a = 0; a < NA; ++a)
#pragma unroll
        for (int t = 0; t < NT; ++t)
#pragma unroll
            for (int r = 0; r < 16; ++r)
                out[(long long)(krow0 + 32 * a + mfma32_row(lane, r)) * s.Cout + n0 + 32 * t + (lane & 31)] = acc[a][t][r];
    if (blockIdx.x == 0) {                                            // bias row: thread's four columns are 4 (tid % (BN/4)); fixed-order sum
        __syncthreads();
        *reinterpret_cast<f32x4*>(&red[tid * 4]) = colsum;
        __syncthreads();
        if (tid < BN) {
            const int grp = tid >> 2, comp = tid & 3;
            float t = 0.f;
            for (int u = grp; u < kWgHaloThreads; u += BN / 4) t += red[u * 4 + comp];
            out[(long long)K * s.Cout + n0 + tid] = t;
        }
    }
}

// ---------------------------------------------------------------------------------------------------------------------
// TS: storage type of X, Y, EPI 3's gate tensor (passed through `bias`) and the pooled-resolution input (convnet.hpp, Chunk4): with
// __bf16 the halo chunks go from global memory to LDS as they are -- no conversion, half the bytes.
// MG: pixel-block rows per item in units of eight (1: 8 x 16 pixels, 2: 16 x 16).  With MG = 2 a wave computes TWO 32-pixel row groups
// against the same weights: the weights of a filter row are staged (L2 -> registers -> LDS) once per 256 pixels instead of once per 128,
// every B fragment read from LDS feeds two MFMAs, and the two barriers of a phase are paid per 48 MFMAs instead of 24 -- for 64 more
// accumulator registers (two workgroups per CU instead of three).
template <int CB, int BN, int EPI, bool PIN = false, typename TS = float, int MG = 1>
__global__ __launch_bounds__(kThreads) __attribute__((amdgpu_waves_per_eu((CB == 64 && BN == 64) || MG == 2 ? 2 : 3))) void k_conv3x3_halo_bf16p(
    const TS* __restrict__ X, const __bf16* __restrict__ WB, const float* __restrict__ bias, TS* __restrict__ Y, ConvShape s, int tiles_w,
    int tiles_h, int n_items, uint8_t* __restrict__ pool_idx, PooledGradT<TS> pin) {
    static_assert(CB % 16 == 0 && BN % 32 == 0, "channel blocks of the 32x32x16 MFMA");
    using Gm = HaloGeom<16, MG>;
    constexpr int TW = 16, NT = BN / 32, LDC = CB + 8;                // halves per pixel / per weight row in LDS (16-byte aligned, bank-skewed)
    constexpr int CPP = CB / 4;                                       // f32x4 chunks per pixel of a channel block
    constexpr int PPW = TW / 2 + 2;                                   // PIN: pooled pixels under the halo: 6 rows x 10
    constexpr int GR = PIN ? Gm::TH / 2 + 2 : Gm::HH, GC = PIN ? PPW : Gm::HWD;    // the grid that is loaded: pooled pixels, or the halo itself
    constexpr int NH = (GR * GC * CPP + kThreads - 1) / kThreads;
    constexpr int BCH = 3 * BN * (CB / 8);                            // 16-byte chunks of one filter row's weights for a channel block
    constexpr int NB = (BCH + kThreads - 1) / kThreads;
    __shared__ __attribute__((aligned(16))) __bf16 Hs[Gm::NPIX * LDC];
    __shared__ __attribute__((aligned(16))) __bf16 Bs[3 * BN * LDC];
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
    const int Cin = s.Cin, K = 9 * Cin, nblk = s.Cout / BN;
    const int GH = PIN ? s.H >> 1 : s.H, GW = PIN ? s.W >> 1 : s.W;   // image size of the loaded grid
    const int r = lane & 31, h = lane >> 5;
    const int py = 2 * wave + (r >> 4), px = r & 15;                  // this lane's A row = output pixel (py, px) of the block

    // work item = (column block nb fastest, block column tw, block row th, image g)
    const ItemWalk walk(nblk, tiles_w, tiles_h);
    auto item_of = [&](const Pos& p) { return Item{p.d3, p.d2 * Gm::TH, p.d1 * TW, p.d0 * BN}; };

    // ---- staging: registers first (loads fly under the MFMAs), LDS after the barrier
    StageMap<NH> hm;
    stage_map_init<NH, GR, GC, 1, CPP>(hm, tid);
    chunk4_t<TS> hv[NH], hp[PIN ? NH : 1];
    unsigned hi[PIN ? NH : 1];
    unsigned okm = 0;
    auto halo_load = [&](const Item& it, int cb) {
        const int y0 = PIN ? (it.oh0 >> 1) - 1 : it.oh0 - 1, x0 = PIN ? (it.ow0 >> 1) - 1 : it.ow0 - 1;
        const int base = ((it.img0 * GH + y0) * GW + x0) * Cin + cb;
        okm = 0;
#pragma unroll
        for (int q = 0; q < NH; ++q) {
            const int pk = opaque(hm.pk[q]);
            const bool ok = stage_ok(pk, y0, x0, it.img0, GH, GW, s.N);
            okm |= (ok ? 1u : 0u) << q;
            const unsigned off = ok ? (unsigned)(base + stage_rel<CPP>(pk, tid, GH, GW, Cin)) : 0u;
            if (PIN) {
                hv[q] = *reinterpret_cast<const chunk4_t<TS>*>(pin.dP + off);
                hp[q] = *reinterpret_cast<const chunk4_t<TS>*>(pin.P + off);
                hi[q] = *reinterpret_cast<const unsigned*>(pin.idx + off);
            } else {
                hv[q] = *reinterpret_cast<const chunk4_t<TS>*>(X + off);
            }
        }
    };
    auto halo_store = [&]() {
        const int c4 = (tid % CPP) * 4;
#pragma unroll
        for (int q = 0; q < NH; ++q) {
            const bool ok = (okm >> q) & 1u;
            const int pk = hm.pk[q];
            if (pk < 0) continue;
            if (PIN) {
                const int pr = pk & 255, pc = (pk >> 8) & 255;
                f32x4 v[4];
                unpool4x4(ok ? widen4(hv[q]) : f32x4{0, 0, 0, 0}, widen4(hp[q]), hi[q], v);
                __bf16* w0 = &Hs[((2 * pr - 1) * Gm::HWD + 2 * pc - 1) * LDC + c4];              // window position 0 (may lie outside the halo)
#pragma unroll
                for (int pos = 0; pos < 4; ++pos) {
                    const bool in = ((pos >> 1) ? pr < Gm::HH / 2 : pr > 0) && ((pos & 1) ? pc < Gm::HWD / 2 : pc > 0);
                    if (in) *reinterpret_cast<bf16x4*>(w0 + ((pos >> 1) * Gm::HWD + (pos & 1)) * LDC) = to_bf16x4(v[pos]);
                }
            } else {
                *reinterpret_cast<bf16x4*>(&Hs[(tid / CPP + (kThreads / CPP) * q) * LDC + c4]) = ok ? to_bf16x4(hv[q]) : bf16x4{(__bf16)0.f, (__bf16)0.f, (__bf16)0.f, (__bf16)0.f};
            }
        }
    };
    // weights of one filter row for a channel block: chunk q of the thread is 8 halves of row (kw * BN + co) of the [3 BN][CB] tile,
    // straight out of the transposed bf16 copy WB[Cout][K].  Row of chunk q = r0 + RQ q with r0 = tid / (CB/8) < RQ and RQ a multiple
    // or a divisor of BN, so (kw, co) of every q is the thread's own (kw0, co0) plus compile-time steps: one register for the global
    // offset, one for the LDS address.
    bf16x8 bv[NB];
    constexpr int RQ = kThreads / (CB / 8);
    static_assert(RQ % BN == 0 || BN % RQ == 0, "rows per step and column block must divide one another");
    const int br0 = tid / (CB / 8), bc8 = (tid % (CB / 8)) * 8;
    const int b_goff = (br0 % BN) * K + (br0 / BN) * Cin + bc8;       // (co0, kw0) of the thread
    const __bf16* const b_lds = &Bs[br0 * LDC + bc8];
    auto b_valid = [&](int q) { return NB * kThreads == BCH || tid + kThreads * q < BCH; };
    auto b_load = [&](const Item& it, int cb, int kh) {
        const __bf16* wp = WB + (long long)it.n0 * K + kh * 3 * Cin + cb + b_goff;
#pragma unroll
        for (int q = 0; q < NB; ++q) {
            // row step RQ q: RQ >= BN: kw += (RQ / BN) q; RQ < BN: co += RQ (q mod BN/RQ), kw += q / (BN/RQ)
            const int dkw = RQ >= BN ? (RQ / BN) * q : q / (BN / RQ), dco = RQ >= BN ? 0 : RQ * (q % (BN / RQ));
            if (b_valid(q)) bv[q] = *reinterpret_cast<const bf16x8*>(wp + (long long)dco * K + dkw * Cin);
        }
    };
    auto b_store = [&]() {
#pragma unroll
        for (int q = 0; q < NB; ++q)
            if (b_valid(q)) *reinterpret_cast<bf16x8*>(const_cast<__bf16*>(b_lds) + RQ * q * LDC) = bv[q];
    };

    const int nph = (Cin / CB) * 3;                                   // phases of one item: (channel block, filter row)
    int item = blockIdx.x;
    if (item >= n_items) return;
    Pos pos = walk.split(item);
    Item cur = item_of(pos);
    halo_load(cur, 0);
    b_load(cur, 0, 0);
    bool first = true;
#pragma unroll 1
    for (; item < n_items; item += gridDim.x) {
        f32x16 acc[MG][NT];
#pragma unroll
        for (int g = 0; g < MG; ++g)
#pragma unroll
            for (int t = 0; t < NT; ++t)
#pragma unroll
                for (int r = 0; r < 16; ++r) acc[g][t][r] = 0.f;
        const int nitem = item + gridDim.x;
        pos = walk.advance(pos);
        const Item nxt = item_of(pos);
        int cb = 0, kh = 0;
#pragma unroll 1
        for (int ph = 0; ph < nph; ++ph) {
            if (!first) __syncthreads();                               // the previous phase's operands have been consumed
            first = false;
            if (kh == 0) halo_store();
            b_store();
            __syncthreads();
            const int nkh = kh == 2 ? 0 : kh + 1, ncb = kh == 2 ? cb + CB : cb;
            // ONE load site for "this item's next phase" and "the next item's first phase": as two sites the compiler loaded the
            // second one into other registers, copied them over behind an s_waitcnt vmcnt(0), and -- those registers doubling as
            // LDS-read destinations -- made every phase wait for most of its just-issued loads BEFORE its MFMAs (ISA, round 4)
            const bool same = ph + 1 < nph;
            const Item li = same ? cur : nxt;
            const int lcb = same ? ncb : 0, lkh = same ? nkh : 0;
            if (same || nitem < n_items) {
                b_load(li, lcb, lkh);
                if (lkh == 0) halo_load(li, lcb);
            }
#pragma unroll
            for (int kw = 0; kw < 3; ++kw) {
                const __bf16* a = &Hs[((py + kh) * Gm::HWD + px + kw) * LDC + 8 * h];
                const __bf16* b = &Bs[(kw * BN + r) * LDC + 8 * h];
#pragma unroll
                for (int ks = 0; ks < CB / 16; ++ks) {
                    bf16x8 af[MG];
#pragma unroll
                    for (int g = 0; g < MG; ++g) af[g] = *reinterpret_cast<const bf16x8*>(a + g * 8 * Gm::HWD * LDC + 16 * ks);
#pragma unroll
                    for (int t = 0; t < NT; ++t) {
                        const bf16x8 bf = *reinterpret_cast<const bf16x8*>(b + 32 * t * LDC + 16 * ks);
#pragma unroll
                        for (int g = 0; g < MG; ++g) acc[g][t] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(af[g], bf, acc[g][t], 0, 0, 0);
                    }
                }
            }
            kh = nkh; cb = ncb;
        }
#pragma unroll
        for (int g = 0; g < MG; ++g) halo_epilogue<TW, NT, EPI, TS, TS>(acc[g], lane, wave, cur.img0, cur.oh0 + 8 * g, cur.ow0, cur.n0, s, bias, Y, pool_idx);
        cur = nxt;
    }
}

// k_conv3x3_halo_bf16_1cb -- the same for layers of exactly 32 input channels (one channel block).  A phase of the kernel above is then
// 6 / 12 MFMAs between two barriers and a restaged weight row -- on the 224 x 224 net's 32-channel layers (6.4 M pixels each) it ran
// at 2.2 x its HBM floor.  Here ALL nine taps' weights of a column block (9 x BN x 32 halves: 23 / 46 KB) are staged once and stay
// while the workgroup walks its items (the column block only changes when the layer has more than BN output channels); an item is its
// halo (prefetched under the previous item's MFMAs), 18 / 36 MFMAs, its epilogue: two barriers per item.
template <int BN, int EPI, bool PIN = false, typename TS = float>
__global__ __launch_bounds__(kThreads) void k_conv3x3_halo_bf16_1cb(const TS* __restrict__ X, const __bf16* __restrict__ WB, const float* __restrict__ bias,
                                                                   TS* __restrict__ Y, ConvShape s, int tiles_w, int tiles_h, int n_items,
                                                                   uint8_t* __restrict__ pool_idx, PooledGradT<TS> pin) {
    using Gm = HaloGeom<16>;
    constexpr int CB = 32, TW = 16, NT = BN / 32, LDC = CB + 8, CPP = CB / 4, K = 9 * CB;
    constexpr int PPW = TW / 2 + 2;
    constexpr int GR = PIN ? 6 : Gm::HH, GC = PIN ? PPW : Gm::HWD;
    constexpr int NH = (GR * GC * CPP + kThreads - 1) / kThreads;
    constexpr int BCH = BN * (K / 8), NB = (BCH + kThreads - 1) / kThreads;          // 16-byte chunks of the column block's weights: 36 per output channel
    __shared__ __attribute__((aligned(16))) __bf16 Hs[Gm::NPIX * LDC];
    __shared__ __attribute__((aligned(16))) __bf16 Bs[9 * BN * LDC];
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
    const int nblk = s.Cout / BN;
    const int GH = PIN ? s.H >> 1 : s.H, GW = PIN ? s.W >> 1 : s.W;
    const int r = lane & 31, h = lane >> 5;
    const int py = 2 * wave + (r >> 4), px = r & 15;

    // work item = (column block nb fastest, block column tw, block row th, image g)
    const ItemWalk walk(nblk, tiles_w, tiles_h);
    auto item_of = [&](const Pos& p) { return Item{p.d3, p.d2 * Gm::TH, p.d1 * TW, p.d0 * BN}; };

    StageMap<NH> hm;
    stage_map_init<NH, GR, GC, 1, CPP>(hm, tid);
    chunk4_t<TS> hv[NH], hp[PIN ? NH : 1];
    unsigned hi[PIN ? NH : 1];
    unsigned okm = 0;
    auto halo_load = [&](const Item& it) {
        const int y0 = PIN ? (it.oh0 >> 1) - 1 : it.oh0 - 1, x0 = PIN ? (it.ow0 >> 1) - 1 : it.ow0 - 1;
        const int base = ((it.img0 * GH + y0) * GW + x0) * CB;
        okm = 0;
#pragma unroll
        for (int q = 0; q < NH; ++q) {
            const int pk = hm.pk[q];
            const bool ok = stage_ok(pk, y0, x0, it.img0, GH, GW, s.N);
            okm |= (ok ? 1u : 0u) << q;
            const unsigned off = ok ? (unsigned)(base + stage_rel<CPP>(pk, tid, GH, GW, CB)) : 0u;
            if (PIN) {
                hv[q] = *reinterpret_cast<const chunk4_t<TS>*>(pin.dP + off);
                hp[q] = *reinterpret_cast<const chunk4_t<TS>*>(pin.P + off);
                hi[q] = *reinterpret_cast<const unsigned*>(pin.idx + off);
            } else {
                hv[q] = *reinterpret_cast<const chunk4_t<TS>*>(X + off);
            }
        }
    };
    auto halo_store = [&]() {
        const int c4 = (tid % CPP) * 4;
#pragma unroll
        for (int q = 0; q < NH; ++q) {
            const bool ok = (okm >> q) & 1u;
            const int pk = hm.pk[q];
            if (pk < 0) continue;
            if (PIN) {
                const int pr = pk & 255, pc = (pk >> 8) & 255;
                f32x4 v[4];
                unpool4x4(ok ? widen4(hv[q]) : f32x4{0, 0, 0, 0}, widen4(hp[q]), hi[q], v);
                __bf16* w0 = &Hs[((2 * pr - 1) * Gm::HWD + 2 * pc - 1) * LDC + c4];
#pragma unroll
                for (int pos = 0; pos < 4; ++pos) {
                    const bool in = ((pos >> 1) ? pr < Gm::HH / 2 : pr > 0) && ((pos & 1) ? pc < Gm::HWD / 2 : pc > 0);
                    if (in) *reinterpret_cast<bf16x4*>(w0 + ((pos >> 1) * Gm::HWD + (pos & 1)) * LDC) = to_bf16x4(v[pos]);
                }
            } else {
                *reinterpret_cast<bf16x4*>(&Hs[(tid / CPP + (kThreads / CPP) * q) * LDC + c4]) = ok ? to_bf16x4(hv[q]) : bf16x4{(__bf16)0.f, (__bf16)0.f, (__bf16)0.f, (__bf16)0.f};
            }
        }
    };
    // the column block's weights: output channel co's nine taps x 32 channels are 288 consecutive halves of WB; chunk e = 8 of them
    auto weights_in = [&](int n0) {
#pragma unroll
        for (int q = 0; q < NB; ++q) {
            const int e = tid + kThreads * q;
            if (NB * kThreads == BCH || e < BCH) {
                const int co = e / (K / 8), j = e - co * (K / 8);
                *reinterpret_cast<bf16x8*>(&Bs[((j >> 2) * BN + co) * LDC + (j & 3) * 8]) = *reinterpret_cast<const bf16x8*>(WB + (long long)(n0 + co) * K + j * 8);
            }
        }
    };

    int item = blockIdx.x;
    if (item >= n_items) return;
    Pos pos = walk.split(item);
    Item cur = item_of(pos);
    halo_load(cur);
    int loaded_n0 = -1;
    float bbr[NT];                                                    // the lane's bias values, loaded with the column block's weights (below)
#pragma unroll
    for (int t = 0; t < NT; ++t) bbr[t] = 0.f;
    bool first = true;
#pragma unroll 1
    for (; item < n_items; item += gridDim.x) {
        f32x16 acc[NT];
#pragma unroll
        for (int t = 0; t < NT; ++t)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[t][r] = 0.f;
        const int nitem = item + gridDim.x;
        pos = walk.advance(pos);
        const Item nxt = item_of(pos);
        if (!first) __syncthreads();                                  // the previous item's operands have been consumed
        first = false;
        if (cur.n0 != loaded_n0) {
            weights_in(cur.n0);
            if (EPI == 1 || EPI == 2 || EPI == 4) {
                // the bias with the weights, complete here: loaded in the epilogue it is the YOUNGEST load, and the wait for it (vmcnt counts
                // in order) is a wait for the next item's halo just prefetched -- every item paid its own prefetch latency (ISA, round 4)
#pragma unroll
                for (int t = 0; t < NT; ++t) bbr[t] = bias[cur.n0 + 32 * t + (lane & 31)];
                __builtin_amdgcn_s_waitcnt(0x0F70);                   // vmcnt(0)
            }
            loaded_n0 = cur.n0;
        }
        halo_store();
        __syncthreads();
        // (EPI 3, one column tile: the gate values are loaded ahead of the MFMAs -- sixteen registers; with two tiles they spill.  Issued
        // BEFORE the prefetch, and the prefetch unconditional (past the last item: this item's halo again, never used): the epilogue's wait
        // for the gates then allows exactly the prefetch's loads to stay in flight)
        constexpr bool GATE_AHEAD = EPI == 3 && NT == 1;
        float gate[NT][16];
        if constexpr (GATE_AHEAD) halo_gate_prefetch<TW, NT, TS>(gate, lane, wave, cur.img0, cur.oh0, cur.ow0, cur.n0, s, reinterpret_cast<const TS*>(bias));
        if (GATE_AHEAD) halo_load(nitem < n_items ? nxt : cur);
        else if (nitem < n_items) halo_load(nxt);
#pragma unroll
        for (int kh = 0; kh < 3; ++kh)
#pragma unroll
            for (int kw = 0; kw < 3; ++kw) {
                const __bf16* a = &Hs[((py + kh) * Gm::HWD + px + kw) * LDC + 8 * h];
                const __bf16* b = &Bs[((kh * 3 + kw) * BN + r) * LDC + 8 * h];
#pragma unroll
                for (int ks = 0; ks < CB / 16; ++ks) {
                    const bf16x8 af = *reinterpret_cast<const bf16x8*>(a + 16 * ks);
#pragma unroll
                    for (int t = 0; t < NT; ++t) {
                        const bf16x8 bf = *reinterpret_cast<const bf16x8*>(b + 32 * t * LDC + 16 * ks);
                        acc[t] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(af, bf, acc[t], 0, 0, 0);
                    }
                }
            }
        __builtin_amdgcn_sched_barrier(0);                            // (nothing of the epilogue -- its waits least of all -- moves in front of the MFMAs)
        halo_epilogue<TW, NT, EPI, TS, TS>(acc, lane, wave, cur.img0, cur.oh0, cur.ow0, cur.n0, s, bias, Y, pool_idx, GATE_AHEAD ? gate : nullptr,
                                           (EPI == 1 || EPI == 2 || EPI == 4) ? bbr : nullptr);
        cur = nxt;
    }
}

}  // namespace rcnx
