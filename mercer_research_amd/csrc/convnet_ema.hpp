// convnet_ema.hpp -- Track X: an exponential moving average of the parameters (rcn_hipx_set_ema), kept by the launch that updates them, and
// the buffer exchange behind an evaluation on it (rcn_hipx_evaluate_ex_dev).  The semantics of timm's ModelEmaV2 and of
// torch.optim.swa_utils.AveragedModel(multi_avg_fn=get_ema_multi_avg_fn(decay)).  No reference counterpart.
//
// Per element, fp32, every operation rounded once (no fused multiply-add):
//     e = e + a * (p_new - e),    a = fl(1.0f - decay), computed once on the host
// p_new being the value the update stores into the parameter buffer in that same step -- torch.lerp(e, p_new, 1 - decay) in its
// weight < 0.5 form; a float32 NumPy restatement reproduces it bit for bit (tests/_ema_ref.py).  Biases are averaged too.  Padding
// elements of the padded layout have p = e = 0 and stay 0.
//
//   WithEma<Update>       wraps an update functor of reduce_all_body: the wrapped update's four new parameters are in registers on their way
//                         to the parameter buffer; the average's four are read, moved towards them and written back.  The parameters pass
//                         through unchanged, so the live parameters, the flipped copy and the velocity are those of a net without an average.
//                         The step's ONE slab reduction carries it: k_reduce_update<.., EMA = true, ..> (convnet_update.hpp).
//   k_ema_lerp            the data-parallel half: the same line over the whole padded buffer, after rcn_hipx_apply_sgd_dev's update launch
//   k_swap4               exchanges two padded buffers (parameters <-> average, around an evaluation on the average)
#pragma once

#include "convnet_sgd.hpp"

namespace rcnx {

struct EmaParams {
    float* e;                 // the average, laid out like the padded parameters
    const float* p0;          // the padded parameter buffer: a job's average is e + (jb.p - p0)
    float a;                  // fl(1 - decay)
};

// four consecutive elements
__device__ __forceinline__ f32x4 ema_update4(const f32x4& e, const f32x4& p, float a) {
#pragma clang fp contract(off)
    const f32x4 d = p - e;
    return e + a * d;
}

// J is only handed on (the wrapped functor reads J.lr): nothing here writes the kernel's argument
template <class Update> struct WithEma {
    Update u;
    EmaParams m;
    __device__ __forceinline__ f32x4 operator()(const ReduceJobs& J, const ReduceJob& jb, long long i, const f32x4& t) const {
        const f32x4 p = u(J, jb, i, t);
        f32x4* ep = reinterpret_cast<f32x4*>(m.e + (jb.p - m.p0) + i);
        *ep = ema_update4(*ep, p, m.a);
        return p;
    }
};

// n % 4 == 0 and e, p 16-byte aligned (host: whole padded buffers)
__global__ void k_ema_lerp(float* __restrict__ e, const float* __restrict__ p, float a, long long n) {
    for (long long i = ((long long)blockIdx.x * blockDim.x + threadIdx.x) * 4; i < n; i += (long long)gridDim.x * blockDim.x * 4) {
        const f32x4 ev = *reinterpret_cast<const f32x4*>(e + i);
        const f32x4 pv = *reinterpret_cast<const f32x4*>(p + i);
        *reinterpret_cast<f32x4*>(e + i) = ema_update4(ev, pv, a);
    }
}

// n % 4 == 0 and a, b 16-byte aligned, distinct buffers (host)
__global__ void k_swap4(float* __restrict__ a, float* __restrict__ b, long long n) {
    for (long long i = ((long long)blockIdx.x * blockDim.x + threadIdx.x) * 4; i < n; i += (long long)gridDim.x * blockDim.x * 4) {
        const f32x4 av = *reinterpret_cast<const f32x4*>(a + i);
        const f32x4 bv = *reinterpret_cast<const f32x4*>(b + i);
        *reinterpret_cast<f32x4*>(a + i) = bv;
        *reinterpret_cast<f32x4*>(b + i) = av;
    }
}

}  // namespace rcnx
