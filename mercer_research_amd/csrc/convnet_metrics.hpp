// convnet_metrics.hpp -- Track X: the evaluation of one chunk of logits (rcn_hipx_evaluate_dev) and what it can tell beyond the loss sum,
// the top-1 count and the arg-max (rcn_hipx_evaluate_metrics_dev).  No reference counterpart.
//
//   k_eval<METRICS, ...>   soft-max cross-entropy, first-maximum arg-max and correct count of one chunk of logits, without d logits; its
//                          last-arriving workgroup ADDS the chunk's totals into a double / int64 pair.  With METRICS, on request, also the
//                          rank of every row's label, top-k counts, the confusion matrix, the per-row loss and a compact copy of the logits.
#pragma once

#include "convnet_loss.hpp"

namespace rcnx {

constexpr int kEvalSamples = 8;        // samples per 256-thread workgroup of k_eval (k_softmax_ce's grouping)
inline int eval_blocks(int B) { return (B + kEvalSamples - 1) / kEvalSamples; }

constexpr int kEvalMaxTopk = 8;        // RCN_HIPX_EVAL_MAX_TOPK
static_assert(kEvalMaxTopk <= kEvalSamples, "k_eval sums the partials of topk[j] with the 32 lanes of sample group j");

// One sample's share of an evaluation, run by the 32 lanes (ln) of its group on its logits row z: the maximum, the FIRST class that
// attains it (ix; written to pred[s] where pred is given), and with labels the label y, loss = -(z[y] - max - log(sum exp)) and
// ok = (ix == y); a label outside [0, C) never indexes the row and leaves loss and ok at the caller's zeros.
__device__ __forceinline__ void eval_sample(const float* __restrict__ z, int C, int ln, const int* __restrict__ labels, int s, int* __restrict__ pred, float& loss, int& ok,
                                            int& ix_out, int& y_out) {
    float mx = -3.0e38f;
    int ix = 0x7fffffff;
    for (int c = ln; c < C; c += 32)
        if (z[c] > mx) { mx = z[c]; ix = c; }           // strictly greater: the first maximum of this lane's classes
#pragma unroll
    for (int off = 16; off > 0; off >>= 1) {
        const float o = __shfl_xor(mx, off, 32);
        const int oi = __shfl_xor(ix, off, 32);
        if (o > mx || (o == mx && oi < ix)) { mx = o; ix = oi; }
    }
    if (ix >= C) ix = 0;                                // (no class above -3e38: a row of NaN or -inf)
    if (pred && ln == 0) pred[s] = ix;
    ix_out = ix;
    if (labels) {
        const int y = labels[s];
        y_out = y;
        if (y >= 0 && y < C) {
            const float sum = row_sum_exp(z, C, ln, mx);
            loss = -(z[y] - mx - logf(sum));
            ok = ix == y;
        }
    }
}

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

// What a metrics launch fills beyond the plain one's results; every pointer is nullable and already moved to the chunk's first row.
// topk_part: [kEvalMaxTopk][part_stride] per-workgroup counts, behind the loss partials, the correct partials and the counter.
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

// Behind eval_sample (its loss, arg-max ix and label y; y < 0 without labels) the 32 lanes of sample s walk the row once more: each copies
// the logits it reads into logits_out and counts the classes that beat the label; a shuffle reduction gives the rank (-1 for a label
// outside [0, C), which indexes nothing and enters no count).  Lane 0 writes loss_each (the float that enters the workgroup's partial)
// and rank, and adds 1 to confusion[y][arg-max] with a vector atomic: integer cells, so the order of the additions cannot change a
// result.  Returns, on lane 0, bit j set where 0 <= rank < topk[j].
__device__ __forceinline__ int eval_sample_metrics(const EvalMetrics& m, const float* __restrict__ z, int C, int ln, bool with_labels, int s, float loss, int ix, int y) {
    const bool ranked = y >= 0 && y < C;
    const float zy = z[ranked ? y : 0];
    float* const out = m.logits_out ? m.logits_out + (long long)s * C : nullptr;
    int above = 0, within = 0;
    for (int c = ln; c < C; c += 32) {
        const float v = z[c];
        if (out) out[c] = v;
        above += beats_label(v, c, zy, y);
    }
#pragma unroll
    for (int off = 16; off > 0; off >>= 1) above += __shfl_xor(above, off, 32);
    const int rank = ranked ? above : -1;
    if (with_labels && ln == 0) {
        if (m.loss_each) m.loss_each[s] = loss;
        if (m.rank) m.rank[s] = rank;
#pragma unroll 1
        for (int j = 0; j < m.n_topk; ++j) within |= (rank >= 0 && rank < m.topk[j]) << j;
        if (m.confusion && ranked) __hip_atomic_fetch_add(&m.confusion[(long long)y * C + ix], 1LL, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
    return within;
}

// Evaluation of one chunk of B logits rows (ldl floats apart): 32 lanes per sample, no d logits.  A label outside [0, C) counts as
// incorrect and adds nothing to the loss (eval_sample).  loss_part[block] = the block's losses summed in sample order, correct_part[block]
// its correct count; the totals by arrive_last / finish_totals.  labels == nullptr: prediction (and logits copy) only, no partials and no
// counter.  METRICS: ONE trailing EvalMetrics argument; thread 0 writes, beside the loss and correct partials, one count per k of the
// workgroup's rows with 0 <= rank < k, and the last workgroup ADDS every k's total into topk_correct.
// In the plans: k_eval<false> is `k_eval_ce`, k_eval<true, EvalMetrics> is `k_eval_metrics`.
template <bool METRICS, typename... M>
__global__ __launch_bounds__(kThreads) void k_eval(const float* __restrict__ logits, const int* __restrict__ labels, int B, int C, int ldl, float* loss_part, int* correct_part,
                                                  unsigned* counter, double* loss_sum, long long* correct, int* __restrict__ pred, M... metrics) {
    __shared__ float red[kEvalSamples];
    __shared__ int hit[kEvalSamples];
    __shared__ int rk[kEvalSamples];                        // (METRICS only)
    const int grp = threadIdx.x >> 5, ln = threadIdx.x & 31;
    const int s = blockIdx.x * kEvalSamples + grp;
    float loss = 0.f;
    int ok = 0, within = 0;
    if (s < B) {
        const float* z = logits + (long long)s * ldl;
        int ix = 0, y = -1;
        eval_sample(z, C, ln, labels, s, pred, loss, ok, ix, y);
        if constexpr (METRICS) within = eval_sample_metrics(metrics..., z, C, ln, labels != nullptr, s, loss, ix, y);
    }
    if (!labels) return;
    if (ln == 0) {
        red[grp] = loss;
        hit[grp] = ok;
        if constexpr (METRICS) rk[grp] = within;
    }
    __syncthreads();
    if (!arrive_last(counter, [&] {
            float t = 0.f;
            int h = 0;
            for (int g = 0; g < kEvalSamples; ++g) { t += red[g]; h += hit[g]; }
            put_partial(loss_part, t);
            put_partial(correct_part, h);
            if constexpr (METRICS) {
                const EvalMetrics m{metrics...};
#pragma unroll 1
                for (int j = 0; j < m.n_topk; ++j) {
                    int in = 0;
                    for (int g = 0; g < kEvalSamples; ++g) in += (rk[g] >> j) & 1;
                    put_partial(m.topk_part + j * m.part_stride, in);
                }
            }
        })) return;
    if constexpr (METRICS) {
        // the top-k partials, all ks at once: group j of 32 lanes sums the partials of topk[j] (lane ln takes blocks ln, ln + 32, ...) and a
        // shuffle reduction adds the 32 sums.  Integers: whatever the order, the total is the same, so this needs neither thread 0's
        // serial sum of 256 per k nor a barrier, and it is under way before that sum of the losses begins.
        const EvalMetrics m{metrics...};
        long long in = 0;
        if (grp < m.n_topk)
            for (int b = ln; b < (int)gridDim.x; b += 32) in += __hip_atomic_load(&m.topk_part[grp * m.part_stride + b], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
#pragma unroll
        for (int off = 16; off > 0; off >>= 1) in += __shfl_xor(in, off, 32);
        if (grp < m.n_topk && ln == 0) m.topk_correct[grp] = m.topk_correct[grp] + in;
    }
    finish_totals(loss_part, correct_part, counter, loss_sum, correct);
}

}  // namespace rcnx
