// convnet_bn.hpp -- Track X: batch normalisation + ReLU behind a bias-only 3x3 convolution (RCN_HIPX_BN_RELU behind RCN_HIPX_CONV3X3),
// and the same with an identity skip added in front of the ReLU (RCN_HIPX_BN_ADD_RELU: k_bn_apply_relu<EVAL, ADD>, k_skip_bwd_add),
// torch.nn.BatchNorm2d(C) followed by ReLU over an NHWC fp32 map x[M][C], M = B * H * W rows, C % 32 == 0.  RCN_HIPX_BN and RCN_HIPX_BN_ADD are
// the same two layers with NO activation (k_bn_apply<EVAL, ADD>: the apply expression without its max(0, .)); their backward pass is the
// ungated form of the kernels below (g = dy as it stands) and their skip's share is never gated.  Every kernel is a streaming
// pass: one thread per FOUR consecutive channels, 16-byte accesses, no atomics of any kind.
//
// The per-channel sums (the statistics of the forward pass, the two sums of the backward pass) are made in two launches:
//   k_bn_stats / k_bn_bwd_reduce   workgroup p of bn_parts(M) takes the rows [p * R, p * R + R), R = bn_rows_per_part(M); thread (r, c)
//                                  adds its rows r, r + RP, ... in double, the RP row lanes of a channel are added in the order 0 .. RP - 1
//                                  and the two partials go to part[p][0 | 1][C] (doubles)
//   k_bn_stats_finish / k_bn_bwd_finish   ONE workgroup of 1024 threads: a team of S = bn_team(C) threads per channel, member j adds the
//                                  partials j, j + S, ... in that order, the members are added in the order 0 .. S - 1, and the first
//                                  member finalises the channel.
// The finalisation is the ONE-WORKGROUP SECOND LAUNCH, not a finished-workgroup counter: nothing to reset, nothing ordered by arrival.
// R, RP, the number of partials and S are functions of (M, C) alone -- never of the grid that happens to be resident -- so every sum has
// ONE order per shape: two nets stepped with the same batches hold the same bits.
//
// Training forward (forward(..., train = true)): with s = sum x, q = sum x^2 (every square exact) in double,
//     mean = s / M              var = max(0, q / M - mean^2)   (biased)           invstd = 1 / sqrt(var + (double)eps)
//     running_mean <- fl32((1 - m) * running_mean + m * mean)                     running_var <- fl32((1 - m) * running_var + m * var * M / (M - 1))
// all in double from the float momentum m; mean and invstd are rounded to float ONCE and saved per layer for the backward pass.
// k_bn_apply_relu, every operation in fp32 and rounded once (no fused multiply-add), in this association:
//     xh = fl(fl(x - mean) * invstd)          y = max(0, fl(fl(xh * gamma) + beta))
// Evaluation forward (rcn_hipx_forward_dev, evaluate*, predict*): the SAME kernel and expression with mean = running_mean and
// invstd = fl32(1 / sqrt((double)running_var + (double)eps)), made by every thread for its four channels -- a per-channel scale and shift
// in the training forward's own rounding order.  weights = "ema" scores the averaged gamma and beta with the LIVE running statistics:
// torch's AveragedModel with use_buffers = False.
//
// Backward: g = dy (already gated by the consumer above), or g = y > 0 ? dy : 0 (GATE: the layer gates itself); xh as above from the
// saved mean and invstd.  k_bn_bwd_reduce sums g and g * xh (the product of the two floats, exact in double) per channel;
// k_bn_bwd_finish rounds the totals to float once into the layer's one-chunk slab [d gamma = sum g xh | d beta = sum g] -- what the
// step's reduction launch and k_bn_bwd_dx both read.  k_bn_bwd_dx, fp32, every operation rounded once:
//     dx = fl(fl(gamma * invstd) * fl(fl(g - fl(sum_g / M)) - fl(xh * fl(sum_gxh / M))))
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "convnet.hpp"

namespace rcnx {

constexpr int kBnThreads = 256;             // the streaming kernels and the partial sums
constexpr int kBnFinishThreads = 1024;      // the one-workgroup second launch
constexpr int kBnMaxParts = 512;            // partials per channel at most: the one finishing workgroup reads 16 * C * parts bytes

// rows per partial (a multiple of 64, at least 64) and the number of partials of a map of M rows: shape alone
__host__ __device__ inline long long bn_rows_per_part(long long M) { const long long r = (M + kBnMaxParts - 1) / kBnMaxParts; return r < 64 ? 64 : (r + 63) / 64 * 64; }
__host__ __device__ inline int bn_parts(long long M) { const long long R = bn_rows_per_part(M); return (int)((M + R - 1) / R); }
// The partials a layer's buffer must hold when its map has AT MOST max_rows rows.  bn_parts is not monotonic -- rows per partial stay 64
// up to 32768 rows (512 partials) and double just above (257) -- so a batch below the largest can need more partials than the largest
// does.  Every M <= max_rows has rows per partial >= 64, hence at most ceil(M / 64) <= ceil(max_rows / 64) partials, and never more than 512.
__host__ __device__ inline int bn_parts_cap(long long max_rows) { const long long p = (max_rows + 63) / 64; return (int)(p < kBnMaxParts ? p : kBnMaxParts); }
// grid.y of the partial kernels: a workgroup covers up to 256 channel groups of four
__host__ __device__ inline int bn_group_blocks(int C) { return (C / 4 + kBnThreads - 1) / kBnThreads; }
// threads per channel of the finishing workgroup: the largest power of two with S * min(C, 1024) <= 1024
__host__ __device__ inline int bn_team(int C) { const int c = C < kBnFinishThreads ? C : kBnFinishThreads; int s = 1; while (2 * s * c <= kBnFinishThreads) s *= 2; return s; }
// workgroups of the streaming kernels over n4 pieces of four channels, at most 4096 and then a few more: a multiple of C4 / gcd(C4, 256),
// so that grid * 256 % C4 == 0 and a thread's four channels never change along its grid-stride loop
inline unsigned bn_stream_blocks(long long n4, int C4) {
    int a = C4, b = kBnThreads;
    while (b) { const int t = a % b; a = b; b = t; }
    const long long q = C4 / a;
    long long g = (n4 + kBnThreads - 1) / kBnThreads;
    if (g > 4096) g = 4096;
    return (unsigned)((g + q - 1) / q * q);
}

__device__ inline f32x4 bn_load4(const float* p) { return *reinterpret_cast<const f32x4*>(p); }
__device__ inline f32x4 bn_invstd_of_var(const f32x4& var, float eps) {
    f32x4 r;
#pragma unroll
    for (int k = 0; k < 4; ++k) r[k] = (float)(1.0 / sqrt((double)var[k] + (double)eps));
    return r;
}
// xh = fl(fl(x - mean) * invstd)
__device__ inline f32x4 bn_xhat(const f32x4& x, const f32x4& mean, const f32x4& invstd) {
#pragma clang fp contract(off)
    f32x4 r;
#pragma unroll
    for (int k = 0; k < 4; ++k) { const float d = x[k] - mean[k]; r[k] = d * invstd[k]; }
    return r;
}

// The two partial sums of workgroup (blockIdx.x: rows, blockIdx.y: 256 channel groups).  Term: `V load(m, c)` fetches what row m, channels
// c .. c + 3 need (four rows are in flight per thread); `add(v, sa, sb)` adds the row's two values per channel, in double.
template <class Term>
__device__ __forceinline__ void bn_partial_body(long long M, int C, double* __restrict__ part, const Term& term) {
    __shared__ double red[kBnThreads][8];
    const int C4 = C / 4;
    const int g0 = (int)blockIdx.y * kBnThreads;
    const int cw = C4 - g0 < kBnThreads ? C4 - g0 : kBnThreads;     // channel groups of this workgroup
    const int RP = kBnThreads / cw;                                  // row lanes (threads past RP * cw idle)
    const int r = (int)threadIdx.x / cw, cg = (int)threadIdx.x % cw;
    const int c = (g0 + cg) * 4;
    const long long R = bn_rows_per_part(M), m0 = (long long)blockIdx.x * R, m1 = m0 + R < M ? m0 + R : M;
    double sa[4] = {0, 0, 0, 0}, sb[4] = {0, 0, 0, 0};
    if (r < RP) {
        long long m = m0 + r;
        for (; m + 3LL * RP < m1; m += 4LL * RP) {
            typename Term::V v[4];
#pragma unroll
            for (int u = 0; u < 4; ++u) v[u] = term.load(m + (long long)u * RP, c);
#pragma unroll
            for (int u = 0; u < 4; ++u) term.add(v[u], sa, sb);
        }
        for (; m < m1; m += RP) term.add(term.load(m, c), sa, sb);
    }
#pragma unroll
    for (int k = 0; k < 4; ++k) { red[threadIdx.x][k] = sa[k]; red[threadIdx.x][4 + k] = sb[k]; }
    __syncthreads();
    if (r == 0) {
        for (int j = 1; j < RP; ++j)
#pragma unroll
            for (int k = 0; k < 4; ++k) { sa[k] += red[j * cw + cg][k]; sb[k] += red[j * cw + cg][4 + k]; }
        double* const pa = part + ((long long)blockIdx.x * 2) * C + c;
#pragma unroll
        for (int k = 0; k < 4; ++k) { pa[k] = sa[k]; pa[C + k] = sb[k]; }
    }
}

// The totals of channel c's two partial columns by its team of S threads of the finishing workgroup (every thread of the workgroup
// calls this): true in the team's first member, which holds the totals.
// Member j = threadIdx.x / per of a channel's team sits `per` threads from the next (per = 1024 / S channels per round), so a wave reads 64
// consecutive doubles of one partial row; eight partial pairs are in flight per thread and added in partial order.  (Measured on the CIFAR
// net, B = 512: with the members of a team in neighbouring lanes and one dependent load per trip this launch took 17 - 60 us, a
// microsecond per trip, more than the streaming pass in front of it.)
__device__ __forceinline__ bool bn_finish_totals(const double* __restrict__ part, int parts, int C, int c, int S, double* ta, double* tb) {
    __shared__ double red[kBnFinishThreads][2];
    const int per = kBnFinishThreads / S, j = (int)threadIdx.x / per;
    double a = 0, b = 0;
    if (c < C)
        for (int p = j; p < parts; p += 8 * S) {
            double va[8], vb[8];
#pragma unroll
            for (int k = 0; k < 8; ++k) {
                const int q = p + k * S;
                va[k] = q < parts ? part[((long long)q * 2) * C + c] : 0.0;
                vb[k] = q < parts ? part[((long long)q * 2 + 1) * C + c] : 0.0;
            }
#pragma unroll
            for (int k = 0; k < 8; ++k) { a += va[k]; b += vb[k]; }
        }
    __syncthreads();                                                  // (the previous round's reads of red)
    red[threadIdx.x][0] = a; red[threadIdx.x][1] = b;
    __syncthreads();
    if (j == 0) for (int k = 1; k < S; ++k) { a += red[threadIdx.x + k * per][0]; b += red[threadIdx.x + k * per][1]; }
    *ta = a; *tb = b;
    return j == 0 && c < C;
}

// ---- training forward: the statistics
struct BnStatsTerm {
    using V = f32x4;
    const float* x; int C;
    __device__ __forceinline__ V load(long long m, int c) const { return bn_load4(x + m * C + c); }
    __device__ __forceinline__ void add(const V& v, double* sa, double* sb) const {
#pragma unroll
        for (int k = 0; k < 4; ++k) { const double d = (double)v[k]; sa[k] += d; sb[k] += d * d; }
    }
};
__global__ __launch_bounds__(kBnThreads) void k_bn_stats(const float* __restrict__ x, long long M, int C, double* __restrict__ part) {
    bn_partial_body(M, C, part, BnStatsTerm{x, C});
}

// mean[C], invstd[C] of the batch (saved for the backward pass) and the running statistics, from the partials
__global__ __launch_bounds__(kBnFinishThreads) void k_bn_stats_finish(const double* __restrict__ part, int parts, long long M, int C, float momentum, float eps,
                                                                       float* __restrict__ mean, float* __restrict__ invstd, float* __restrict__ run_mean, float* __restrict__ run_var) {
    const int S = bn_team(C), per = kBnFinishThreads / S;
    for (int c0 = 0; c0 < C; c0 += per) {
        const int c = c0 + (int)threadIdx.x % per;
        double s, q;
        if (!bn_finish_totals(part, parts, C, c, S, &s, &q)) continue;
        const double mu = s / (double)M;
        double var = q / (double)M - mu * mu;
        if (var < 0) var = 0;
        mean[c] = (float)mu;
        invstd[c] = (float)(1.0 / sqrt(var + (double)eps));
        const double m = (double)momentum;
        run_mean[c] = (float)((1.0 - m) * (double)run_mean[c] + m * mu);
        run_var[c] = (float)((1.0 - m) * (double)run_var[c] + m * (var * (double)M / (double)(M - 1)));
    }
}

// y = max(0, fl(fl(xh * gamma) + beta)), xh = fl(fl(x - mean) * invstd); EVAL: stat2 is the running variance, else the batch's invstd.
// ADD (RCN_HIPX_BN_ADD_RELU): y = max(0, fl(fl(fl(xh * gamma) + beta) + s)), s the skip's map, loaded as 16 bytes beside x
// ADD 2 (RCN_HIPX_BN_ADD_RELU_DOWN): s is the output of a layer of twice the height and width and Cs <= C channels, added through the
// parameter-free option-A shortcut s'[b][h][w][c] = s[b][2h][2w][c - lo] for lo <= c < lo + Cs, else 0: one 16-byte load at the strided
// pixel where the thread's four channels lie in the window (lo % 4 == 0 and Cs % 4 == 0: never split), zeros elsewhere
struct SkipDown { int oH, oW, Cs, lo; };      // this layer's map; the source's channels; the first channel of the window
__device__ inline SkipDown skip_geom() { return SkipDown{}; }
__device__ inline SkipDown skip_geom(const SkipDown& d) { return d; }
// DOWN...: empty (RCN_HIPX_BN_RELU, RCN_HIPX_BN_ADD_RELU: the kernel's arguments are what they were), or one SkipDown behind eps
// RELU false (RCN_HIPX_BN, RCN_HIPX_BN_ADD: k_bn_apply): the same expression without the max(0, .), y = fl(fl(xh * gamma) + beta) [+ s]
template <bool EVAL, bool ADD, bool RELU, class... DOWN>
__device__ __forceinline__ void bn_apply_body(const float* __restrict__ x, const float* __restrict__ s, float* __restrict__ y, long long n4, int C,
                                              const float* __restrict__ mean, const float* __restrict__ stat2, const float* __restrict__ gamma,
                                              const float* __restrict__ beta, float eps, DOWN... down) {
#pragma clang fp contract(off)
    const int C4 = C / 4;
    long long e = (long long)blockIdx.x * kBnThreads + threadIdx.x;
    if (e >= n4) return;
    const int c = (int)(e % C4) * 4;                                 // (the grid's threads are a multiple of C4: bn_stream_blocks)
    const f32x4 mu = bn_load4(mean + c), ga = bn_load4(gamma + c), be = bn_load4(beta + c);
    f32x4 is = bn_load4(stat2 + c);
    if (EVAL) is = bn_invstd_of_var(is, eps);
    for (; e < n4; e += (long long)gridDim.x * kBnThreads) {
        const f32x4 xv = bn_load4(x + e * 4);
        f32x4 sv;
        if (ADD && sizeof...(DOWN) == 0) sv = bn_load4(s + e * 4);
        if constexpr (sizeof...(DOWN) == 1) {
            const SkipDown d = skip_geom(down...);
            const long long px = e / C4;
            const int w = (int)(px % d.oW);
            const long long t = px / d.oW;
            const int h = (int)(t % d.oH);
            const long long b = t / d.oH;
            const bool in = c >= d.lo && c < d.lo + d.Cs;
            const f32x4 v = bn_load4(s + (in ? ((b * (2 * d.oH) + 2 * h) * (2 * d.oW) + 2 * w) * d.Cs + (c - d.lo) : 0));      // unconditional load, masked by value
            sv = in ? v : f32x4{0.f, 0.f, 0.f, 0.f};
        }
        const f32x4 xh = bn_xhat(xv, mu, is);
        f32x4 v;
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const float t = xh[k] * ga[k];
            float u = t + be[k];
            if (ADD) u = u + sv[k];
            v[k] = RELU ? (u > 0.f ? u : 0.f) : u;
        }
        *reinterpret_cast<f32x4*>(y + e * 4) = v;
    }
}
template <bool EVAL, bool ADD, class... DOWN>
__global__ __launch_bounds__(kBnThreads) void k_bn_apply_relu(const float* __restrict__ x, const float* __restrict__ s, float* __restrict__ y, long long n4, int C,
                                                              const float* __restrict__ mean, const float* __restrict__ stat2, const float* __restrict__ gamma,
                                                              const float* __restrict__ beta, float eps, DOWN... down) {
    bn_apply_body<EVAL, ADD, true>(x, s, y, n4, C, mean, stat2, gamma, beta, eps, down...);
}
// RCN_HIPX_BN (ADD false) and RCN_HIPX_BN_ADD (identity skip): batch normalisation with no activation behind it
template <bool EVAL, bool ADD>
__global__ __launch_bounds__(kBnThreads) void k_bn_apply(const float* __restrict__ x, const float* __restrict__ s, float* __restrict__ y, long long n4, int C,
                                                         const float* __restrict__ mean, const float* __restrict__ stat2, const float* __restrict__ gamma,
                                                         const float* __restrict__ beta, float eps) {
    bn_apply_body<EVAL, ADD, false>(x, s, y, n4, C, mean, stat2, gamma, beta, eps);
}

// ---- backward
template <bool GATE> struct BnBwdTerm {
    struct V { f32x4 x, g, y; };
    const float* x; const float* dy; const float* y; const float* mean; const float* invstd; int C;
    __device__ __forceinline__ V load(long long m, int c) const {
        V v;
        v.x = bn_load4(x + m * C + c); v.g = bn_load4(dy + m * C + c);
        if (GATE) v.y = bn_load4(y + m * C + c);
        return v;
    }
    f32x4 mu, is;                                                     // the thread's four channels (set by the kernel)
    __device__ __forceinline__ void add(const V& v, double* sa, double* sb) const {
        const f32x4 xh = bn_xhat(v.x, mu, is);
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const float g = (!GATE || v.y[k] > 0.f) ? v.g[k] : 0.f;
            sa[k] += (double)g * (double)xh[k]; sb[k] += (double)g;
        }
    }
};
// part[p][0][C] = sum g * xh, part[p][1][C] = sum g over the rows of partial p
template <bool GATE>
__global__ __launch_bounds__(kBnThreads) void k_bn_bwd_reduce(const float* __restrict__ x, const float* __restrict__ dy, const float* __restrict__ y, long long M, int C,
                                                              const float* __restrict__ mean, const float* __restrict__ invstd, double* __restrict__ part) {
    const int C4 = C / 4, g0 = (int)blockIdx.y * kBnThreads;
    const int cw = C4 - g0 < kBnThreads ? C4 - g0 : kBnThreads;
    const int c = (g0 + (int)threadIdx.x % cw) * 4;                   // bn_partial_body's own channel of this thread
    BnBwdTerm<GATE> t{x, dy, y, mean, invstd, C, bn_load4(mean + c), bn_load4(invstd + c)};
    bn_partial_body(M, C, part, t);
}
// the layer's one-chunk slab [d gamma | d beta], floats
__global__ __launch_bounds__(kBnFinishThreads) void k_bn_bwd_finish(const double* __restrict__ part, int parts, int C, float* __restrict__ slab) {
    const int S = bn_team(C), per = kBnFinishThreads / S;
    for (int c0 = 0; c0 < C; c0 += per) {
        const int c = c0 + (int)threadIdx.x % per;
        double sgx, sg;
        if (!bn_finish_totals(part, parts, C, c, S, &sgx, &sg)) continue;
        slab[c] = (float)sgx;
        slab[C + c] = (float)sg;
    }
}
// dx = fl(fl(gamma * invstd) * fl(fl(g - fl(sum_g / M)) - fl(xh * fl(sum_gxh / M))))
template <bool GATE>
__global__ __launch_bounds__(kBnThreads) void k_bn_bwd_dx(const float* __restrict__ x, const float* __restrict__ dy, const float* __restrict__ y, float* __restrict__ dx, long long n4,
                                                          int C, float m_rows, const float* __restrict__ mean, const float* __restrict__ invstd, const float* __restrict__ gamma,
                                                          const float* __restrict__ slab) {
#pragma clang fp contract(off)
    const int C4 = C / 4;
    long long e = (long long)blockIdx.x * kBnThreads + threadIdx.x;
    if (e >= n4) return;
    const int c = (int)(e % C4) * 4;
    const f32x4 mu = bn_load4(mean + c), is = bn_load4(invstd + c), ga = bn_load4(gamma + c);
    const f32x4 sgx = bn_load4(slab + c), sg = bn_load4(slab + C + c);
    f32x4 k0, k1, k2;
#pragma unroll
    for (int k = 0; k < 4; ++k) { k0[k] = ga[k] * is[k]; k1[k] = sg[k] / m_rows; k2[k] = sgx[k] / m_rows; }
    for (; e < n4; e += (long long)gridDim.x * kBnThreads) {
        const f32x4 xh = bn_xhat(bn_load4(x + e * 4), mu, is);
        f32x4 g = bn_load4(dy + e * 4);
        if (GATE) {
            const f32x4 yv = bn_load4(y + e * 4);
#pragma unroll
            for (int k = 0; k < 4; ++k) g[k] = yv[k] > 0.f ? g[k] : 0.f;
        }
        f32x4 v;
#pragma unroll
        for (int k = 0; k < 4; ++k) { const float a = g[k] - k1[k]; const float b = xh[k] * k2[k]; const float d = a - b; v[k] = k0[k] * d; }
        *reinterpret_cast<f32x4*>(dx + e * 4) = v;
    }
}

// ---- the skip's half of a RCN_HIPX_BN_ADD_RELU layer's backward pass: the gradient of the sum, g = dy of that layer (GATE_SELF: gated
// here with its output, y_self > 0; else it arrived gated), added to the gradient of the skip's source once the input-gradient kernel of
// the layer above the source has written it:
//     dsrc = fl(dsrc + g)         GATE_SRC: g counts only where y_src > 0 -- dsrc already is the source's dZ, and the skip's share
//                                 passes the same gate
// One thread per four floats, every element read and written by the same thread, grid-stride, no atomics: one order, one result.
template <bool GATE_SELF, bool GATE_SRC>
__global__ __launch_bounds__(kBnThreads) void k_skip_bwd_add(float* __restrict__ dsrc, const float* __restrict__ dy, const float* __restrict__ y_self,
                                                             const float* __restrict__ y_src, long long n4) {
    for (long long e = (long long)blockIdx.x * kBnThreads + threadIdx.x; e < n4; e += (long long)gridDim.x * kBnThreads) {
        f32x4 a = bn_load4(dsrc + e * 4);
        f32x4 g = bn_load4(dy + e * 4);
        if (GATE_SELF) {
            const f32x4 yv = bn_load4(y_self + e * 4);
#pragma unroll
            for (int k = 0; k < 4; ++k) g[k] = yv[k] > 0.f ? g[k] : 0.f;
        }
        if (GATE_SRC) {
            const f32x4 yv = bn_load4(y_src + e * 4);
#pragma unroll
            for (int k = 0; k < 4; ++k) g[k] = yv[k] > 0.f ? g[k] : 0.f;
        }
#pragma unroll
        for (int k = 0; k < 4; ++k) a[k] = a[k] + g[k];
        *reinterpret_cast<f32x4*>(dsrc + e * 4) = a;
    }
}
// The same for a RCN_HIPX_BN_ADD_RELU_DOWN layer: one thread per four floats of the SMALL map's Cs-channel window,
//     dsrc[b][2h][2w][c'] = fl(dsrc[b][2h][2w][c'] + g[b][h][w][c' + lo])
// with the identity skip's gate table, the source's gate read at the strided position.  A quarter of the source map is touched, each
// element by one thread.  n4 = B * oH * oW * Cs / 4; C: the channels of dy and y_self.
template <bool GATE_SELF, bool GATE_SRC>
__global__ __launch_bounds__(kBnThreads) void k_skip_bwd_add_down(float* __restrict__ dsrc, const float* __restrict__ dy, const float* __restrict__ y_self,
                                                                  const float* __restrict__ y_src, long long n4, int C, SkipDown d) {
    const int Cs4 = d.Cs / 4;
    for (long long e = (long long)blockIdx.x * kBnThreads + threadIdx.x; e < n4; e += (long long)gridDim.x * kBnThreads) {
        const int c = (int)(e % Cs4) * 4;
        const long long px = e / Cs4;
        const int w = (int)(px % d.oW);
        const long long t = px / d.oW;
        const int h = (int)(t % d.oH);
        const long long b = t / d.oH;
        const long long so = ((b * (2 * d.oH) + 2 * h) * (2 * d.oW) + 2 * w) * d.Cs + c, go = px * C + d.lo + c;
        f32x4 a = bn_load4(dsrc + so);
        f32x4 g = bn_load4(dy + go);
        if (GATE_SELF) {
            const f32x4 yv = bn_load4(y_self + go);
#pragma unroll
            for (int k = 0; k < 4; ++k) g[k] = yv[k] > 0.f ? g[k] : 0.f;
        }
        if (GATE_SRC) {
            const f32x4 yv = bn_load4(y_src + so);
#pragma unroll
            for (int k = 0; k < 4; ++k) g[k] = yv[k] > 0.f ? g[k] : 0.f;
        }
#pragma unroll
        for (int k = 0; k < 4; ++k) a[k] = a[k] + g[k];
        *reinterpret_cast<f32x4*>(dsrc + so) = a;
    }
}

}  // namespace rcnx
