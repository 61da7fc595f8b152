// convnet_sgd.hpp -- Track X: SGD with momentum, weight decay and Nesterov (rcn_hipx_set_sgd), the semantics of torch.optim.SGD with
// dampening 0.  No reference counterpart.
//
// Per element, fp32, in this order (weight decay applies to every parameter, biases included):
//     d = grad_scale * g
//     if wd != 0:  d = d + wd * p
//     if mu != 0:  v = mu * v + d;   d = nesterov ? d + mu * v : v          (v starts at 0: step 1 gives v = d)
//     p = p - lr * d
// Every operation rounds once (no fused multiply-add), so a float32 NumPy restatement reproduces it bit for bit
// (tests/_sgd_ref.py).  Padding elements of the padded layout have g = p = v = 0 and stay 0.
//
//   SgdUpdate         an update functor of reduce_all_body: this update in place of p <- p - lr g in the step's ONE slab reduction
//                     (k_reduce_update<.., OPT = kOptSgd, ..>, convnet_update.hpp), the training step of a net with a non-default setting.
//                     The tap-flipped weight copy is kept current as with PlainUpdate.
//   k_sgd_apply       the data-parallel half: the same update from an all-reduced padded gradient buffer, grid-stride, 16-byte accesses.
#pragma once

#include "convnet.hpp"

namespace rcnx {

struct SgdParams {
    float* v;                 // velocity, laid out like the padded parameters; nullptr when mu == 0 and no buffer exists
    const float* p0;          // the padded parameter buffer: a job's velocity is v + (jb.p - p0)
    float mu, wd;
    int nesterov;
};

// four consecutive elements; v is read and written only when mu != 0
__device__ __forceinline__ void sgd_update4(f32x4& p, f32x4& v, const f32x4& g, float grad_scale, float lr, const SgdParams& s) {
#pragma clang fp contract(off)
    f32x4 d = grad_scale * g;
    if (s.wd != 0.f) d = d + s.wd * p;
    if (s.mu != 0.f) {
        v = s.mu * v + d;
        d = s.nesterov ? d + s.mu * v : v;
    }
    p = p - lr * d;
}

struct SgdUpdate {
    SgdParams s;
    __device__ __forceinline__ f32x4 operator()(const ReduceJobs& J, const ReduceJob& jb, long long i, const f32x4& t) const {
        f32x4 p = *reinterpret_cast<const f32x4*>(jb.p + i);
        if (s.mu != 0.f) {
            f32x4* vp = reinterpret_cast<f32x4*>(s.v + (jb.p - s.p0) + i);
            f32x4 v = *vp;
            sgd_update4(p, v, t, 1.f, J.lr, s);
            *vp = v;
        } else {
            f32x4 none = {0.f, 0.f, 0.f, 0.f};
            sgd_update4(p, none, t, 1.f, J.lr, s);
        }
        return p;
    }
};

// n % 4 == 0 and p, v, g 16-byte aligned (host)
__global__ void k_sgd_apply(float* __restrict__ p, const float* __restrict__ g, float grad_scale, float lr, SgdParams s, long long n) {
    for (long long i = ((long long)blockIdx.x * blockDim.x + threadIdx.x) * 4; i < n; i += (long long)gridDim.x * blockDim.x * 4) {
        f32x4 pv = *reinterpret_cast<const f32x4*>(p + i);
        const f32x4 gv = *reinterpret_cast<const f32x4*>(g + i);
        if (s.mu != 0.f) {
            f32x4 vv = *reinterpret_cast<const f32x4*>(s.v + i);
            sgd_update4(pv, vv, gv, grad_scale, lr, s);
            *reinterpret_cast<f32x4*>(s.v + i) = vv;
        } else {
            f32x4 none = {0.f, 0.f, 0.f, 0.f};
            sgd_update4(pv, none, gv, grad_scale, lr, s);
        }
        *reinterpret_cast<f32x4*>(p + i) = pv;
    }
}

}  // namespace rcnx
