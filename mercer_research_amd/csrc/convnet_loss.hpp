// convnet_loss.hpp -- Track X: soft-max cross-entropy, written once for the kernels that compute it.  No reference counterpart.
//
//   row_max / row_sum_exp      one logits row under the 32 lanes of its sample: the training loss and the evaluation (convnet_metrics.hpp)
//   SoftTarget, soft_*         label smoothing and / or a weighted pair of labels: the training loss and k_head_f32<.., SOFT> (convnet_halo.hpp)
//   arrive_last, finish_*      per-workgroup partials summed by the workgroup that arrives LAST, in a fixed order: all five kernels
//   k_softmax_ce<SOFT, ...>    fused softmax + cross-entropy forward and (p - target) / B backward
#pragma once

#include "convnet.hpp"

namespace rcnx {

// ---- one logits row z of C classes under 32 lanes: lane ln takes classes ln, ln + 32, ...; every lane returns the row's value
__device__ __forceinline__ float row_max(const float* __restrict__ z, int C, int ln) {
    float mx = -3.0e38f;
    for (int c = ln; c < C; c += 32) mx = z[c] > mx ? z[c] : mx;
#pragma unroll
    for (int off = 16; off > 0; off >>= 1) { const float o = __shfl_xor(mx, off, 32); mx = o > mx ? o : mx; }
    return mx;
}
__device__ __forceinline__ float row_sum_exp(const float* __restrict__ z, int C, int ln, float mx) {
    float sum = 0.f;
    for (int c = ln; c < C; c += 32) sum += expf(z[c] - mx);
#pragma unroll
    for (int off = 16; off > 0; off >>= 1) sum += __shfl_xor(sum, off, 32);
    return sum;
}

// ---- the soft target.  What a soft-target loss takes beyond the hard one's labels (rcn_hipx_set_loss, rcn_hipx_train_step_pair_dev):
//     t_c = (1 - eps) * (w * [c == ya] + (1 - w) * [c == yb]) + eps / C
// labels_b == nullptr: yb = ya; weight (ONE device scalar, the weight of the row's own label ya) == nullptr: w = 1.
struct SoftTarget { const int* labels_b; const float* weight; float eps; };
struct SoftCoef { float keep, w, wb, u; };              // 1 - eps, w, 1 - w, eps / C

// With lp_c = (z_c - mx) - logf(sum), every operation rounded once (no fused multiply-add):
//     loss = -((1 - eps) * (w * lp_ya + (1 - w) * lp_yb) + (eps / C) * sum_c lp_c)        d_c = (p_c - t_c) * inv_b
// A label outside [0, C) never indexes the row: its indicator is 0 everywhere and its lp term is dropped (the evaluation's rule).  At
// eps = 0, w = 1 the expressions give the hard loss's bits without a special case: 1 * x, x + 0 and 0 * x (x finite) are exact.
__device__ __forceinline__ SoftCoef soft_coef(SoftTarget tg, int C) {
#pragma clang fp contract(off)
    const float w = tg.weight ? *tg.weight : 1.f;
    return SoftCoef{1.f - tg.eps, w, 1.f - w, tg.eps / (float)C};
}
// lpa, lpb: lp of the two labels (0: outside [0, C)); slp: the sum of lp_c over the classes
__device__ __forceinline__ float soft_loss_of(const SoftCoef& k, float lpa, float lpb, float slp) {
#pragma clang fp contract(off)
    return -(k.keep * (k.w * lpa + k.wb * lpb) + k.u * slp);
}
__device__ __forceinline__ float soft_t(const SoftCoef& k, int c, int ya, int yb) {
#pragma clang fp contract(off)
    return k.keep * (k.w * (c == ya ? 1.f : 0.f) + k.wb * (c == yb ? 1.f : 0.f)) + k.u;
}

// ---- the last-arriver sum: every workgroup leaves partials at part[blockIdx.x]; the one that arrives LAST (a counter beside the
// partials, which it leaves at zero for the next launch) adds them in block order -- no second launch, and the sum does not depend on
// which workgroup that was.
template <typename T> __device__ __forceinline__ void put_partial(T* part, T v) { __hip_atomic_store(&part[blockIdx.x], v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }

// Thread 0 runs publish() -- the workgroup's samples added in group order, put_partial for each sum -- and arrives; every thread learns
// whether this workgroup is the last.  All threads call it, behind a barrier that covers what publish() reads.
template <typename Publish> __device__ __forceinline__ bool arrive_last(unsigned* counter, Publish publish) {
    __shared__ int last;
    if (threadIdx.x == 0) {
        publish();
        last = __hip_atomic_fetch_add(counter, 1u, __ATOMIC_ACQ_REL, __HIP_MEMORY_SCOPE_AGENT) == gridDim.x - 1;
    }
    __syncthreads();
    return last;
}

// The last workgroup of a training kernel (kThreads threads; red: kThreads floats of LDS): thread t takes blocks t, t + kThreads, ...,
// thread 0 adds the kThreads sums in index order, *loss_out = total * inv_b.  loss_out == nullptr: no partial is read and only the counter is written
// (the barriers stay: this is k_head_f32's form, whose code must not move).
__device__ __forceinline__ void finish_mean(const float* loss_part, unsigned* counter, float inv_b, float* __restrict__ loss_out, float* red) {
    const int tid = threadIdx.x;
    float t = 0.f;
    if (loss_out)
        for (int b = tid; b < (int)gridDim.x; b += kThreads) t += __hip_atomic_load(&loss_part[b], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    __syncthreads();
    red[tid] = t;
    __syncthreads();
    if (tid == 0) {
        float tot = 0.f;
        for (int i = 0; i < kThreads; ++i) tot += red[i];
        if (loss_out) *loss_out = tot * inv_b;
        __hip_atomic_store(counter, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
}

// The last workgroup of an evaluation kernel: the same order in double / long long, ADDED into *loss_sum / *correct -- chunks run one
// after the other on the net's stream, so the accumulators need no atomics.
__device__ __forceinline__ void finish_totals(const float* loss_part, const int* correct_part, unsigned* counter, double* loss_sum, long long* correct) {
    __shared__ double dsum[kThreads];
    __shared__ long long csum[kThreads];
    double t = 0.0;
    long long h = 0;
    for (int b = threadIdx.x; b < (int)gridDim.x; b += kThreads) {
        t += (double)__hip_atomic_load(&loss_part[b], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        h += __hip_atomic_load(&correct_part[b], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
    dsum[threadIdx.x] = t;
    csum[threadIdx.x] = h;
    __syncthreads();
    if (threadIdx.x == 0) {
        double tot = 0.0;
        long long hits = 0;
        for (int i = 0; i < kThreads; ++i) { tot += dsum[i]; hits += csum[i]; }
        *loss_sum = *loss_sum + tot;
        *correct = *correct + hits;
        __hip_atomic_store(counter, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
}

// fused softmax + cross-entropy: 32 lanes per sample (the padded logits row is ldl wide), eight samples per 256-thread workgroup.
// loss_part[block] = sum of the block's losses in sample order; *loss_out = their mean (finish_mean).
// (One thread per sample -- three serial passes over the classes on two CUs -- took 11 us for 512 samples, plus 5 us for the
// one-thread k_sum_small behind it.)
// In the plans: k_softmax_ce<false> is `k_softmax_ce`, loss = -lp_y; k_softmax_ce<true, SoftTarget> is `k_softmax_ce_soft`, which takes its
// target from ONE trailing SoftTarget argument.
template <bool SOFT, typename... Soft>
__global__ __launch_bounds__(kThreads) void k_softmax_ce(const float* __restrict__ logits, const int* __restrict__ labels, int B, int C, int ldl, float* __restrict__ dlogits,
                                                        float* loss_part, unsigned* counter, float inv_b, float* __restrict__ loss_out, Soft... soft) {
    __shared__ float red[kThreads];
    const int grp = threadIdx.x >> 5, ln = threadIdx.x & 31;
    const int s = blockIdx.x * 8 + grp;
    float loss = 0.f;
    if (s < B) {
        const float* z = logits + (long long)s * ldl;
        if constexpr (SOFT) {
#pragma clang fp contract(off)
            const SoftTarget tg{soft...};
            const int ya = labels[s], yb = tg.labels_b ? tg.labels_b[s] : ya;
            const SoftCoef k = soft_coef(tg, C);
            const float mx = row_max(z, C, ln), sum = row_sum_exp(z, C, ln, mx), lse = logf(sum);
            float slp = 0.f;
            for (int c = ln; c < C; c += 32) slp += (z[c] - mx) - lse;
#pragma unroll
            for (int off = 16; off > 0; off >>= 1) slp += __shfl_xor(slp, off, 32);
            const float lpa = (ya >= 0 && ya < C) ? (z[ya] - mx) - lse : 0.f;
            const float lpb = (yb >= 0 && yb < C) ? (z[yb] - mx) - lse : 0.f;
            loss = soft_loss_of(k, lpa, lpb, slp);
            if (dlogits) {
                float* d = dlogits + (long long)s * ldl;
                for (int c = ln; c < ldl; c += 32) {
                    const float t = soft_t(k, c, ya, yb);
                    d[c] = c < C ? (expf(z[c] - mx) / sum - t) * inv_b : 0.f;
                }
            }
        } else {
            const int y = labels[s];
            const float mx = row_max(z, C, ln), sum = row_sum_exp(z, C, ln, mx);
            loss = -(z[y] - mx - logf(sum));
            if (dlogits) {
                float* d = dlogits + (long long)s * ldl;
                for (int c = ln; c < ldl; c += 32) d[c] = c < C ? (expf(z[c] - mx) / sum - (c == y ? 1.f : 0.f)) * inv_b : 0.f;
            }
        }
    }
    if (ln == 0) red[grp] = loss;
    __syncthreads();
    if (!arrive_last(counter, [&] {
            float t = 0.f;
            for (int g = 0; g < 8; ++g) t += red[g];
            put_partial(loss_part, t);
        })) return;
    finish_mean(loss_part, counter, inv_b, loss_out, red);
}

}  // namespace rcnx
