// convnet_pw.hpp -- Track X: the 1x1 convolution (RCN_HIPX_CONV1X1) as a streaming GEMM with a short contraction.
//
// On an NHWC map a 1x1 convolution is Y[m][co] = sum_k X[m][k] W[k][co] over M = N H W rows with K = Cin = 32 .. 512: one to sixteen
// K-tiles, far below the ridge with bf16 operands and at or below it in fp32.  What the layer costs is reading X and writing Y, so:
//
//   * the weights are staged ONCE per workgroup: the whole [K][NB] slice sits in LDS before the first row is touched and stays there
//     (no per-K-tile restaging, no split-K).  NB = Cout where K x Cout fits the slice (pw_slice_elems), so X is read exactly once per
//     launch; else gridDim.y = Cout / NB workgroup columns each read X once ("passes");
//   * the A operand never touches LDS: a lane loads 16-byte pieces of ITS OWN row of X straight into the registers the MFMA reads.
//     The MFMA lane (r, h) = (lane & 31, lane >> 5) owns row r; which k a lane contracts in which MFMA is free as long as A and B
//     agree, so per 8 channels lane (r, h) loads channels 8 g + 4 h .. + 3 in one piece and MFMA j of the group contracts the pair
//     {8 g + j, 8 g + 4 + j} (fp32, 32x32x2); with bf16 operands the natural layout already is eight consecutive k per lane
//     (32x32x16: k = 16 i + 8 h + 0 .. 7 -- two pieces).  No tap offsets, no border tests; the only row predicate is m < M, applied
//     as an address clamp on the loads (a row past M contracts garbage nobody stores) and as the store predicate;
//   * a resident grid: workgroup (bx, by) takes row blocks bx, bx + gridDim.x, ... of 128 rows (a wave owns 32).  Its work is the
//     sequence of steps (row block, 32-channel K-tile); the loads of steps s + 1 .. s + 3 are in flight while step s is contracted
//     (a ring of four register stages, 3 x 64 bytes per lane under every 16 / 2 MFMAs), across row-block boundaries too;
//   * no coupling between workgroups: no flags, no atomics; every element of Y is written once by one thread in one fixed
//     summation order (k-tiles ascending, within a tile the MFMA order above), so two runs give the same bits.
//
// Both directions of the layer run here: forward X W + b (EPI 1), input gradient dZ Wt (EPI 0 raw / 3 gated by G > 0, `bias` = G shaped
// like Y) on the flipped copy, which for a 1x1 filter is the plain transpose [Cout][Cin] -- again a [K'][Cout'] row-major matrix.
// bf16: the weights come from the prepared bf16 copies [Cout'][K'] (k-contiguous), X is rounded to bf16 (RNE) on its way into the MFMA.
//
// LDS image: fp32 [K][NB + 8] floats (lanes h = 0 / 1 read rows four apart: 4 (NB + 8) = 32 mod 64 banks, the two halves of a wave
// never meet); bf16 [NB][K + 8] halves (16-byte rows 2 K + 16 bytes apart, as convnet_bf16.hpp's tiles).  Dynamic, at most 80 KB:
// two workgroups per CU of 160 KB.  Registers: 16 NB / 32 accumulators + 4 x 16 staged + addresses; NB <= 256 -> <= 128 + 64 + ~30.
#pragma once

#include "convnet.hpp"
#include "convnet_bf16.hpp"

namespace rcnx {

constexpr int kPwRows = 128;                 // rows of X per row block (32 per wave)
constexpr int kPwStages = 4;                 // register stages of one 32-channel K-tile each
constexpr int kPwMaxNB = 256;                // widest column slice (eight 32x32 accumulators per wave)
constexpr int kPwPad32 = 8, kPwPad16 = 8;    // LDS row padding: floats ([K][NB + 8]) / halves ([NB][K + 8])
// elements of W one workgroup keeps in LDS: 64 KB of either precision before padding
__host__ __device__ constexpr long long pw_slice_elems(bool bf16) { return bf16 ? 32768 : 16384; }
__host__ __device__ inline size_t pw_lds_bytes(bool bf16, int K, int NB) {
    return bf16 ? (size_t)NB * (K + kPwPad16) * sizeof(__bf16) : (size_t)K * (NB + kPwPad32) * sizeof(float);
}

extern __shared__ __attribute__((aligned(16))) unsigned char pw_lds_raw[];

// X[M][K] (row-major, K % 32 == 0), W: fp32 Wk[K][Cout] or bf16 WB[Cout][K]; Y[M][Cout]; NT = NB / 32 accumulator tiles per wave.
// grid (row-block workgroups, Cout / NB), 256 threads, dynamic LDS pw_lds_bytes(BF16, K, 32 NT).
template <bool BF16, int NT, int EPI>
__global__ __launch_bounds__(kThreads) __attribute__((amdgpu_waves_per_eu(NT <= 4 ? 2 : 1))) void k_pw(const float* __restrict__ X, const void* __restrict__ Wv, const float* __restrict__ bias,
                                                 float* __restrict__ Y, long long M, int K, int Cout) {
    constexpr int NB = 32 * NT;
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63, r = lane & 31, h = lane >> 5;
    const int n0 = blockIdx.y * NB;
    const int nkt = K / kBK;
    float* const Wf = reinterpret_cast<float*>(pw_lds_raw);
    __bf16* const Wh = reinterpret_cast<__bf16*>(pw_lds_raw);
    const int ldf = NB + kPwPad32, ldh = K + kPwPad16;

    // ---- the weights, once
    if constexpr (BF16) {
        const __bf16* WB = reinterpret_cast<const __bf16*>(Wv);
        const int k8 = K / 8;
        for (int e = tid; e < NB * k8; e += kThreads) {
            const int col = e / k8, kq = e - col * k8;
            *reinterpret_cast<bf16x8*>(Wh + col * ldh + kq * 8) = *reinterpret_cast<const bf16x8*>(WB + (long long)(n0 + col) * K + kq * 8);
        }
    } else {
        const float* Wk = reinterpret_cast<const float*>(Wv);
        for (int e = tid; e < K * (NB / 4); e += kThreads) {
            const int k = e / (NB / 4), c4 = (e - k * (NB / 4)) * 4;
            *reinterpret_cast<f32x4*>(Wf + k * ldf + c4) = *reinterpret_cast<const f32x4*>(Wk + (long long)k * Cout + n0 + c4);
        }
    }

    // ---- the steps of this workgroup: (its j-th row block, K-tile kt), s = j nkt + kt
    const long long nblocks = (M + kPwRows - 1) / kPwRows;
    const int mine = blockIdx.x < nblocks ? (int)((nblocks - blockIdx.x + gridDim.x - 1) / gridDim.x) : 0;
    const int steps = mine * nkt;
    f32x4 st[kPwStages][4];
    // the loader's and the contraction's own place in the sequence: first row of the row block and K-tile (no division per step)
    const long long block_rows = (long long)gridDim.x * kPwRows;
    long long lm0 = (long long)blockIdx.x * kPwRows, cm0 = lm0;
    int lkt = 0, ckt = 0;
    // a lane's four 16-byte pieces of the next step: fp32 channels 32 kt + 8 g + 4 h, g = 0 .. 3; bf16 channels 32 kt + 16 i + 8 h + {0, 4}
    auto load = [&](f32x4 (&v)[4]) {
        long long m = lm0 + wave * 32 + r;
        m = m < M ? m : M - 1;                                         // the row predicate, as an address clamp
        const float* p = X + m * (long long)K + lkt * kBK + (BF16 ? 8 * h : 4 * h);
#pragma unroll
        for (int g = 0; g < 4; ++g) v[g] = *reinterpret_cast<const f32x4*>(p + (BF16 ? 16 * (g >> 1) + 4 * (g & 1) : 8 * g));
        if (++lkt == nkt) { lkt = 0; lm0 += block_rows; }
    };
    f32x16 acc[NT];
    auto contract = [&](const f32x4 (&v)[4]) {
        const int kt = ckt;
        if (kt == 0) {
#pragma unroll
            for (int t = 0; t < NT; ++t)
#pragma unroll
                for (int q = 0; q < 16; ++q) acc[t][q] = 0.f;
        }
        if constexpr (BF16) {
            const __bf16* b = Wh + r * ldh + kt * kBK + 8 * h;
#pragma unroll
            for (int i = 0; i < 2; ++i) {
                const bf16x4 lo = to_bf16x4(v[2 * i]), hi = to_bf16x4(v[2 * i + 1]);
                const bf16x8 af = {lo[0], lo[1], lo[2], lo[3], hi[0], hi[1], hi[2], hi[3]};
#pragma unroll
                for (int t = 0; t < NT; ++t) {
                    const bf16x8 bf = *reinterpret_cast<const bf16x8*>(b + 32 * t * ldh + 16 * i);
                    acc[t] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(af, bf, acc[t], 0, 0, 0);
                }
            }
        } else {
            const float* b = Wf + (kt * kBK + 4 * h) * ldf + r;
#pragma unroll
            for (int g = 0; g < 4; ++g)
#pragma unroll
                for (int q = 0; q < 4; ++q) {
                    const float af = v[g][q];
#pragma unroll
                    for (int t = 0; t < NT; ++t) acc[t] = __builtin_amdgcn_mfma_f32_32x32x2f32(af, b[(8 * g + q) * ldf + 32 * t], acc[t], 0, 0, 0);
                }
        }
        if (kt == nkt - 1) {
            // the row block is whole: lane holds column n0 + 32 t + r, rows mfma32_row(lane, q)
            const long long m0 = cm0 + wave * 32;
#pragma unroll
            for (int t = 0; t < NT; ++t) {
                const int co = n0 + 32 * t + r;
                const float bb = EPI == 1 ? bias[co] : 0.f;
#pragma unroll
                for (int q = 0; q < 16; ++q) {
                    const long long m = m0 + mfma32_row(lane, q);
                    if (m < M) {
                        float y = acc[t][q] + bb;
                        if (EPI == 3) y = bias[m * Cout + co] > 0.f ? y : 0.f;
                        Y[m * Cout + co] = y;
                    }
                }
            }
            ckt = 0; cm0 += block_rows;
        } else ++ckt;
    };

#pragma unroll
    for (int u = 0; u < kPwStages - 1; ++u)
        if (u < steps) load(st[u]);
    __syncthreads();                                                   // the weights are in LDS
    for (int s = 0; s < steps; s += kPwStages) {
#pragma unroll
        for (int u = 0; u < kPwStages; ++u) {
            if (s + u < steps) {
                if (s + u + kPwStages - 1 < steps) load(st[(u + kPwStages - 1) % kPwStages]);
                contract(st[u]);
            }
        }
    }
}

}  // namespace rcnx
