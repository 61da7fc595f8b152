// convnet_clip.hpp -- Track X: gradient clipping by global L2 norm (rcn_hipx_set_clip), the semantics of
// torch.nn.utils.clip_grad_norm_(params, max_norm, norm_type=2, error_if_nonfinite=False) over all parameters, biases included, with the
// norm as a logged quantity.  No reference counterpart.
//
// With g the step's summed gradient in the padded flat layout (n floats, n % 4 == 0; padding elements are 0) and `scale` a factor (1 inside
// the training step).  fp32 unless it says double, every operation rounded once (no fused multiply-add):
//     x_i        = fl(scale * g_i)
//     block b    = elements [4096 b, 4096 b + 4096); missing ones count as 0; thread t of 1024 owns elements 4t .. 4t + 3 of its block
//     s_t        = ((double)x0*x0 + (double)x1*x1) + ((double)x2*x2 + (double)x3*x3)
//     partial[b] = the 1024 s_t combined by the halving tree: strides 512, 256, .., 1; s[t] += s[t + stride] for t < stride
//     S          = acc[t] = partial[t] + partial[t + 1024] + ... (increasing index, in double), then the same tree over acc[0 .. 1024)
//     norm       = (float)sqrt(S)                                 double square root, one rounding to float
//     coef       = min(1.0f, max_norm / (norm + 1e-6f))           a NaN quotient stays NaN, as torch.clamp(max=1) keeps it
//     g'_i       = fl(coef * x_i)                                 always multiplied, as torch does; coef == 1 changes no bit
// g' is what the configured update (convnet_sgd.hpp, with the average of convnet_ema.hpp behind it) sees as its gradient; weight decay is
// added after clipping.  Values are never inspected.  tests/_clip_ref.py restates all of it in NumPy, bit for bit.
//
//   k_grad_sumsq         partial[b] of every block of a buffer: no atomics, no counters, no fences -- a function of the buffer alone
//   clip_coef_all        every workgroup of the launch that applies the coefficient sums the partials in the fixed order above (a few KB
//                        from L2) and gets the same bits: no grid-wide hand-off.  Workgroup 0, thread 0 also records (norm, coef), the
//                        ring log's slot and the step counter with plain stores: one writer, stream-ordered.
//   Clipped<Update>      wraps an update functor of reduce_all_body: hands it fl(coef * t) and returns its parameters
//   k_reduce_update<CLIP = true, ..>   (convnet_update.hpp)
//                        the clipped update launch over the net's gradient buffer, each layer's slice a one-chunk slab, so the flipped
//                        weight copy, the velocity and the average are kept exactly as the unclipped launch keeps them.  The plain and the
//                        configured optimiser do NOT share an instantiation: PlainUpdate's p - lr * g compiles to one fused multiply-add
//                        (the unclipped step and k_axpy have always rounded it once), SgdUpdate with mu = wd = 0 rounds the product and the
//                        difference, and a measure-only step (max_norm = +inf) has to leave an unclipped step's bits.
//   k_sgd_apply_clip<PLAIN>
//                        the data-parallel half: k_sgd_apply with d = fl(coef * fl(grad_scale * g)); PLAIN (the default optimiser):
//                        p = fma(-lr, d, p), the one rounding of PlainUpdate
//   k_grad_norm_finish   one workgroup: the norm of a buffer's partials into a caller's device float (rcn_hipx_grad_norm_dev)
#pragma once

#include "convnet_ema.hpp"

namespace rcnx {

constexpr int kClipThreads = 1024;                       // == kReduceThreads: clip_coef_all runs inside the reduction launch
constexpr int kClipBlockElems = 4 * kClipThreads;
static_assert(kClipThreads == kReduceThreads, "the clipped update launch sums the partials with the reduction's workgroup");

__host__ __device__ inline long long clip_blocks(long long n) { return (n + kClipBlockElems - 1) / kClipBlockElems; }

// the halving tree over s[0 .. 1024); the result is s[0] after the last barrier
__device__ __forceinline__ double clip_tree(double* s) {
    for (int st = kClipThreads >> 1; st >= 1; st >>= 1) {
        __syncthreads();
        if ((int)threadIdx.x < st) s[threadIdx.x] += s[threadIdx.x + st];
    }
    __syncthreads();
    return s[0];
}

// n % 4 == 0 and g 16-byte aligned (host); one workgroup per 4096 elements
__global__ __launch_bounds__(kClipThreads) void k_grad_sumsq(const float* __restrict__ g, long long n, float scale, double* __restrict__ partial) {
#pragma clang fp contract(off)
    __shared__ double s[kClipThreads];
    const long long i = (long long)blockIdx.x * kClipBlockElems + (long long)threadIdx.x * 4;
    f32x4 x = {0.f, 0.f, 0.f, 0.f};
    if (i < n) x = scale * *reinterpret_cast<const f32x4*>(g + i);
    const double x0 = x[0], x1 = x[1], x2 = x[2], x3 = x[3];
    s[threadIdx.x] = (x0 * x0 + x1 * x1) + (x2 * x2 + x3 * x3);
    const double total = clip_tree(s);
    if (threadIdx.x == 0) partial[blockIdx.x] = total;
}

struct ClipNorm { float norm, coef; };

// S of partial[0 .. nblk) by a workgroup of 1024 threads (all of them call this)
__device__ __forceinline__ double clip_total(const double* __restrict__ partial, int nblk) {
#pragma clang fp contract(off)
    __shared__ double acc[kClipThreads];
    double a = 0.0;
    for (int b = threadIdx.x; b < nblk; b += kClipThreads) a = a + partial[b];
    acc[threadIdx.x] = a;
    return clip_tree(acc);
}

__device__ __forceinline__ ClipNorm clip_norm_coef(double S, float max_norm) {
#pragma clang fp contract(off)
    const float norm = (float)sqrt(S);
    const float q = max_norm / (norm + 1e-6f);
    return ClipNorm{norm, q > 1.0f ? 1.0f : q};
}

struct ClipParams {
    const double* partial;    // k_grad_sumsq's, of the gradient this launch applies
    int nblk;
    float max_norm;
    float* out;               // the net's (norm, coef) of the last clipped update
    float* log;               // ring of `cap` norms, or nullptr
    long long cap;
    unsigned long long* count;     // clipped updates since the log was set
};

// the coefficient of this launch, the same bits in every workgroup; workgroup 0 records it
__device__ __forceinline__ float clip_coef_all(const ClipParams& c) {
    const ClipNorm r = clip_norm_coef(clip_total(c.partial, c.nblk), c.max_norm);
    if (blockIdx.x == 0 && threadIdx.x == 0) {
        c.out[0] = r.norm;
        c.out[1] = r.coef;
        const unsigned long long k = *c.count;
        if (c.log) c.log[k % (unsigned long long)c.cap] = r.norm;
        *c.count = k + 1;
    }
    return r.coef;
}

// J is only handed on (the wrapped functor reads J.lr): nothing here writes the kernel's argument
template <class Update> struct Clipped {
    Update u;
    float coef;
    __device__ __forceinline__ f32x4 operator()(const ReduceJobs& J, const ReduceJob& jb, long long i, const f32x4& t) const {
#pragma clang fp contract(off)
        const f32x4 c = coef * t;
        return u(J, jb, i, c);
    }
};

// n % 4 == 0 and p, v, g 16-byte aligned (host); workgroups of 1024 threads
template <bool PLAIN>
__global__ __launch_bounds__(kClipThreads) void k_sgd_apply_clip(float* __restrict__ p, const float* __restrict__ g, float grad_scale, float lr, SgdParams s, long long n, ClipParams C) {
#pragma clang fp contract(off)
    const float coef = clip_coef_all(C);
    for (long long i = ((long long)blockIdx.x * blockDim.x + threadIdx.x) * 4; i < n; i += (long long)gridDim.x * blockDim.x * 4) {
        f32x4 pv = *reinterpret_cast<const f32x4*>(p + i);
        const f32x4 x = grad_scale * *reinterpret_cast<const f32x4*>(g + i);
        const f32x4 gv = coef * x;
        if constexpr (PLAIN) {
#pragma unroll
            for (int k = 0; k < 4; ++k) pv[k] = __builtin_fmaf(-lr, gv[k], pv[k]);
        } else if (s.mu != 0.f) {
            f32x4 vv = *reinterpret_cast<const f32x4*>(s.v + i);
            sgd_update4(pv, vv, gv, 1.f, lr, s);
            *reinterpret_cast<f32x4*>(s.v + i) = vv;
        } else {
            f32x4 none = {0.f, 0.f, 0.f, 0.f};
            sgd_update4(pv, none, gv, 1.f, lr, s);
        }
        *reinterpret_cast<f32x4*>(p + i) = pv;
    }
}

// one workgroup of 1024 threads
__global__ __launch_bounds__(kClipThreads) void k_grad_norm_finish(const double* __restrict__ partial, int nblk, float* __restrict__ norm) {
    const double S = clip_total(partial, nblk);
    if (threadIdx.x == 0) *norm = clip_norm_coef(S, 0.f).norm;
}

}  // namespace rcnx
