// convnet_adam.hpp -- Track X: Adam and AdamW (rcn_hipx_set_adam), the semantics of torch.optim.Adam(betas, eps, weight_decay) in its L2
// form and of torch.optim.AdamW (decoupled decay), amsgrad and maximize off.  No reference counterpart.
//
// Host constants, computed once at configuration, in float: b1 = (float)beta1, b2 = (float)beta2, a1 = fl(1.0f - b1), a2 = fl(1.0f - b2),
// eps, wd.  Device state, the 32-byte AdamTick: the update's ordinal and what the bias corrections need of it.  It starts at step = 0,
// b1t = b2t = 1.0.  The tick, once per update, in double (running products, not pow: a double multiply and the double sqrt reproduce in
// NumPy bit for bit, a device pow does not):
//     step += 1;  b1t = b1t * (double)b1;  b2t = b2t * (double)b2;
//     c1 = (float)(1.0 - b1t);  c2 = (float)sqrt(1.0 - b2t)
// Per element, fp32, in this order (weight decay applies to every parameter, biases included); lr is the step's rate:
//     x = g
//     if wd != 0 and !decoupled:  x = x + wd * p
//     if wd != 0 and  decoupled:  p = p * (1.0f - lr * wd)          (the factor rounded twice: the product, the difference)
//     m = m + a1 * (x - m)                                          (torch's lerp form)
//     v = b2 * v + a2 * (x * x)
//     d = sqrtf(v) / c2 + eps
//     p = p - (lr / c1) * (m / d)
// Every operation rounds once (no fused multiply-add; IEEE sqrtf and /: the library is built without fast-math), so a float32 NumPy
// restatement reproduces it bit for bit (tests/_adam_ref.py).  Padding elements of the padded layout have g = p = m = v = 0 and stay 0.
//
//   k_adam_tick       one workgroup, one thread: the tick, a launch of its own directly in front of the update launch.  A training step is
//                     a replayed graph whose kernel arguments are frozen, so the ordinal lives on the device; and every workgroup of the
//                     update launch has to see the SAME c1 and c2, so the launch that reads them cannot also advance them (a workgroup
//                     that starts late would read the next update's) -- the clip counter's one-thread read-and-increment does not carry over.
//   AdamUpdate        an update functor of reduce_all_body: this update in place of p <- p - lr g in the step's ONE slab reduction
//                     (k_reduce_update<.., OPT = kOptAdam, ..>, convnet_update.hpp).  c1 and c2 are two uniform loads per thread.
//   k_adam_apply<CLIP>
//                     the data-parallel half: the same update from an all-reduced padded gradient buffer, x = fl(grad_scale * g), and with
//                     CLIP fl(coef * x) through clip_coef_all as k_sgd_apply_clip does; grid-stride, 16-byte accesses.
#pragma once

#include "convnet_clip.hpp"

namespace rcnx {

struct AdamTick {
    long long step;           // updates so far
    double b1t, b2t;          // b1^step, b2^step as running products in double
    float c1, c2;             // (float)(1 - b1t), (float)sqrt(1 - b2t): the bias corrections of update `step`
};
static_assert(sizeof(AdamTick) == 32, "AdamTick is 32 bytes");

// host and device: one tick, the arithmetic above (the host rebuilds the state from a step count with it, rcn_hipx_set_adam_state)
__host__ __device__ inline void adam_tick(AdamTick& t, float b1, float b2) {
#pragma clang fp contract(off)
    t.step += 1;
    t.b1t = t.b1t * (double)b1;
    t.b2t = t.b2t * (double)b2;
    t.c1 = (float)(1.0 - t.b1t);
    t.c2 = (float)sqrt(1.0 - t.b2t);
}

struct AdamParams {
    float* m;                 // first and second moment, laid out like the padded parameters
    float* v;
    const float* p0;          // the padded parameter buffer: a job's moments are m + (jb.p - p0), v + (jb.p - p0)
    const AdamTick* tick;     // advanced by k_adam_tick in front of this launch
    float b1, b2, a1, a2, eps, wd;
    int decoupled;
};

// four consecutive elements
__device__ __forceinline__ void adam_update4(f32x4& p, f32x4& m, f32x4& v, const f32x4& g, float lr, float c1, float c2, const AdamParams& a) {
#pragma clang fp contract(off)
    f32x4 x = g;
    if (a.wd != 0.f) {
        if (a.decoupled) {
            const float lw = lr * a.wd;
            const float f = 1.0f - lw;
            p = p * f;
        } else x = x + a.wd * p;
    }
    const f32x4 xm = x - m;
    m = m + a.a1 * xm;
    const f32x4 xx = x * x;
    v = a.b2 * v + a.a2 * xx;
    const float s = lr / c1;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const float d = sqrtf(v[k]) / c2 + a.eps;
        const float q = m[k] / d;
        p[k] = p[k] - s * q;
    }
}

struct AdamUpdate {
    AdamParams a;
    __device__ __forceinline__ f32x4 operator()(const ReduceJobs& J, const ReduceJob& jb, long long i, const f32x4& t) const {
        f32x4 p = *reinterpret_cast<const f32x4*>(jb.p + i);
        f32x4* mp = reinterpret_cast<f32x4*>(a.m + (jb.p - a.p0) + i);
        f32x4* vp = reinterpret_cast<f32x4*>(a.v + (jb.p - a.p0) + i);
        f32x4 m = *mp, v = *vp;
        adam_update4(p, m, v, t, J.lr, a.tick->c1, a.tick->c2, a);
        *mp = m;
        *vp = v;
        return p;
    }
};

__global__ void k_adam_tick(AdamTick* t, float b1, float b2) {
    if (blockIdx.x == 0 && threadIdx.x == 0) {
        AdamTick s = *t;
        adam_tick(s, b1, b2);
        *t = s;
    }
}

// n % 4 == 0 and p, m, v, g 16-byte aligned (host); workgroups of 1024 threads
template <bool CLIP>
__global__ __launch_bounds__(kClipThreads) void k_adam_apply(float* __restrict__ p, const float* __restrict__ g, float grad_scale, float lr, AdamParams a, long long n, ClipParams C) {
#pragma clang fp contract(off)
    float coef = 1.f;
    if constexpr (CLIP) coef = clip_coef_all(C);
    const float c1 = a.tick->c1, c2 = a.tick->c2;
    for (long long i = ((long long)blockIdx.x * blockDim.x + threadIdx.x) * 4; i < n; i += (long long)gridDim.x * blockDim.x * 4) {
        f32x4 pv = *reinterpret_cast<const f32x4*>(p + i);
        f32x4 gv = grad_scale * *reinterpret_cast<const f32x4*>(g + i);
        if constexpr (CLIP) gv = coef * gv;
        f32x4 mv = *reinterpret_cast<const f32x4*>(a.m + i);
        f32x4 vv = *reinterpret_cast<const f32x4*>(a.v + i);
        adam_update4(pv, mv, vv, gv, lr, c1, c2, a);
        *reinterpret_cast<f32x4*>(a.m + i) = mv;
        *reinterpret_cast<f32x4*>(a.v + i) = vv;
        *reinterpret_cast<f32x4*>(p + i) = pv;
    }
}

}  // namespace rcnx
