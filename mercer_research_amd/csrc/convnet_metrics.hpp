// convnet_metrics.hpp -- Track X: what an evaluation can tell beyond the loss sum, the top-1 count and the arg-max
// (rcn_hipx_evaluate_metrics_dev).  No reference counterpart.
//
//   k_eval_metrics   k_eval_ce's launch over one chunk of logits with, on request, the rank of every row's label, top-k counts, the
//                    confusion matrix, the per-row loss and a compact copy of the logits.  The loss, the arg-max and the correct count
//                    are eval_sample's (convnet_epoch.hpp), the routine k_eval_ce runs, summed in k_eval_ce's order: the same bits.
#pragma once

#include "convnet_epoch.hpp"

namespace rcnx {

constexpr int kEvalMaxTopk = 8;        // RCN_HIPX_EVAL_MAX_TOPK
static_assert(kEvalMaxTopk <= kEvalSamples, "k_eval_metrics sums the partials of topk[j] with the 32 lanes of sample group j");

// Class c with logit v BEATS the label y with logit zy: a larger logit, or the same logit at a smaller index -- the label's place in a
// stable descending sort, and the first-maximum rule of the arg-max (rank 0 exactly where the arg-max is the label).  A NaN beats nothing
// and is beaten by nothing.
__host__ __device__ inline bool beats_label(float v, int c, float zy, int y) { return v > zy || (v == zy && c < y); }

// the function the kernel runs, on the host (rcn_hipx_label_rank): how many classes beat the label; -1 for a label outside [0, C)
inline int label_rank(const float* z, int C, int y) {
    if (y < 0 || y >= C) return -1;
    int r = 0;
    for (int c = 0; c < C; ++c) r += beats_label(z[c], c, z[y], y);
    return r;
}

// What a metrics launch fills beyond k_eval_ce's results; every pointer is nullable and already moved to the chunk's first row.
// topk_part: [kEvalMaxTopk][part_stride] per-workgroup counts, beside the loss and correct partials in the metrics launch's own buffer.
struct EvalMetrics {
    int n_topk;
    int topk[kEvalMaxTopk];
    int* topk_part;
    int part_stride;
    long long* topk_correct;           // [n_topk] accumulators
    long long* confusion;              // [C][C] accumulators, row = label, column = arg-max
    float* loss_each;                  // [B]
    int* rank;                         // [B]
    float* logits_out;                 // [B][C] compact
};

// k_eval_ce with more outputs: the same grid, the same 32 lanes per sample, the same partials and the same last-arriving workgroup.
// After eval_sample the 32 lanes walk the row once more: each copies the logits it reads into logits_out and counts the classes that beat
// the label; a shuffle reduction gives the rank (-1 for a label outside [0, C), which indexes nothing and enters no count).  Lane 0 of the
// sample writes loss_each (the float that enters the workgroup's partial) and rank, and adds 1 to confusion[y][arg-max] with a vector
// atomic: integer cells, so the order of the additions cannot change a result.  Thread 0 writes, beside the loss and correct partials,
// one count per k of the workgroup's rows with 0 <= rank < k; the last-arriving workgroup, behind the loss and correct sums it makes in
// k_eval_ce's order, sums every k's partials (32 lanes per k) and ADDS the totals into topk_correct.  labels == nullptr: arg-max and
// logits copy only.
__global__ __launch_bounds__(256) void k_eval_metrics(const float* __restrict__ logits, const int* __restrict__ labels, int B, int C, int ldl, float* loss_part, int* correct_part,
                                                      unsigned* counter, double* loss_sum, long long* correct, int* __restrict__ pred, EvalMetrics m) {
    __shared__ float red[kEvalSamples];
    __shared__ int hit[kEvalSamples];
    __shared__ int rk[kEvalSamples];
    __shared__ double dsum[256];
    __shared__ long long csum[256];
    __shared__ int last;
    const int grp = threadIdx.x >> 5, ln = threadIdx.x & 31;
    const int s = blockIdx.x * kEvalSamples + grp;
    float loss = 0.f;
    int ok = 0, rank = -1, within = 0;                      // within: bit j set where 0 <= rank < topk[j]
    if (s < B) {
        const float* z = logits + (long long)s * ldl;
        int ix = 0, y = -1;
        eval_sample(z, C, ln, labels, s, pred, loss, ok, ix, y);
        const bool ranked = y >= 0 && y < C;                // (y stays -1 without labels)
        const float zy = z[ranked ? y : 0];
        float* const out = m.logits_out ? m.logits_out + (long long)s * C : nullptr;
        int above = 0;
        for (int c = ln; c < C; c += 32) {
            const float v = z[c];
            if (out) out[c] = v;
            above += beats_label(v, c, zy, y);
        }
#pragma unroll
        for (int off = 16; off > 0; off >>= 1) above += __shfl_xor(above, off, 32);
        if (ranked) rank = above;
        if (labels && ln == 0) {
            if (m.loss_each) m.loss_each[s] = loss;
            if (m.rank) m.rank[s] = rank;
#pragma unroll 1
            for (int j = 0; j < m.n_topk; ++j) within |= (rank >= 0 && rank < m.topk[j]) << j;
            if (m.confusion && ranked) __hip_atomic_fetch_add(&m.confusion[(long long)y * C + ix], 1LL, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        }
    }
    if (!labels) return;
    if (ln == 0) { red[grp] = loss; hit[grp] = ok; rk[grp] = within; }
    __syncthreads();
    if (threadIdx.x == 0) {
        float t = 0.f;
        int h = 0;
        for (int g = 0; g < kEvalSamples; ++g) { t += red[g]; h += hit[g]; }
        __hip_atomic_store(&loss_part[blockIdx.x], t, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        __hip_atomic_store(&correct_part[blockIdx.x], h, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
#pragma unroll 1
        for (int j = 0; j < m.n_topk; ++j) {
            int in = 0;
            for (int g = 0; g < kEvalSamples; ++g) in += (rk[g] >> j) & 1;
            __hip_atomic_store(&m.topk_part[j * m.part_stride + blockIdx.x], in, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        }
        last = __hip_atomic_fetch_add(counter, 1u, __ATOMIC_ACQ_REL, __HIP_MEMORY_SCOPE_AGENT) == gridDim.x - 1;
    }
    __syncthreads();
    if (!last) return;
    // the top-k partials, all ks at once: group j of 32 lanes sums the partials of topk[j] (lane ln takes blocks ln, ln + 32, ...) and a
    // shuffle reduction adds the 32 sums.  Integers: whatever the order, the total is the same, so this needs neither thread 0's
    // serial sum of 256 per k nor a barrier, and it is under way before that sum of the losses begins.
    long long in = 0;
    if (grp < m.n_topk)
        for (int b = ln; b < (int)gridDim.x; b += 32) in += __hip_atomic_load(&m.topk_part[grp * m.part_stride + b], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
#pragma unroll
    for (int off = 16; off > 0; off >>= 1) in += __shfl_xor(in, off, 32);
    if (grp < m.n_topk && ln == 0) m.topk_correct[grp] = m.topk_correct[grp] + in;
    double t = 0.0;
    long long h = 0;
    for (int b = threadIdx.x; b < (int)gridDim.x; b += 256) {
        t += (double)__hip_atomic_load(&loss_part[b], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        h += __hip_atomic_load(&correct_part[b], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
    dsum[threadIdx.x] = t;
    csum[threadIdx.x] = h;
    __syncthreads();
    if (threadIdx.x == 0) {
        double tot = 0.0;
        long long hits = 0;
        for (int i = 0; i < 256; ++i) { tot += dsum[i]; hits += csum[i]; }
        *loss_sum = *loss_sum + tot;
        *correct = *correct + hits;
    }
    if (threadIdx.x == 0) __hip_atomic_store(counter, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

}  // namespace rcnx
