// convnet_dropout.hpp -- Track X: inverted dropout behind every RCN_HIPX_DENSE_RELU layer (rcn_hipx_set_dropout), the semantics of
// torch.nn.Dropout(p) in training mode; the draw is the library's own counter-based one, not torch's stream.  No reference counterpart
// (SURVEY.md §0).
//
// Host constants, computed once at configuration: s = fl(1.0f / fl(1.0f - p)); thr = (uint32_t)llrint((double)p * 16777216.0), so a drop
// has probability thr / 2^24.  Site d is the d-th RCN_HIPX_DENSE_RELU layer in layer order, from 0.  Element idx = r * U + u of site d (row
// r < B, unit u < U) draws in the training forward with ordinal t, in wrapping 64-bit arithmetic (splitmix64's finaliser, as k_gather_aug):
//     z = seed ^ (t * 0xD1342543DE82EF95);   z += ((((uint64)d << 48) + idx) + 1) * 0x9E3779B97F4A7C15
//     z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9;  z = (z ^ (z >> 27)) * 0x94D049BB133111EB;  z ^= z >> 31
//     keep = (uint32)(z >> 40) >= thr
// Forward, in place in the layer's output buffer directly behind its forward launch: a' = keep ? fl(a * s) : +0.0f.  Everything downstream
// reads a', and since s >= 1 is finite a' > 0 holds exactly when the element was kept and a > 0: the ReLU gates that compare that buffer
// with 0 (launch_conv's epilogue 3, k_head_f32<GATE>) already apply the mask to the gradient that comes back.  Backward, in place in the
// site layer's dout directly behind the launch that wrote the gated gradient g: fl(g * s).  Every operation rounds once.
//
//   k_dropout_tick    one workgroup, one thread: t += 1, the first launch of every training forward while p > 0.  A training step is a
//                     replayed graph whose kernel arguments are frozen, so the ordinal lives on the device (as k_adam_tick's does).
//   k_dropout_fwd     one thread per four consecutive units (U % 32 == 0: 16-byte loads and stores), 256 threads per workgroup; t through
//                     the device pointer (or, t_dev == nullptr, the explicit t of rcn_hipx_dropout_apply_dev); the draw in 64-bit integer
//                     VALU, no LDS, no mask in memory; (d << 48) + r * U hoisted out of the four draws.
//   k_dropout_bwd     the in-place scale, same shape.
#pragma once

#include "convnet.hpp"

namespace rcnx {

constexpr int kDropThreads = 256;

// the part of the draw that a launch shares: seed and ordinal
__host__ __device__ inline unsigned long long dropout_stem(unsigned long long seed, unsigned long long t) { return seed ^ (t * 0xD1342543DE82EF95ull); }
// host and device: is element q = (site << 48) + idx kept?  (rcn_hipx_dropout_draw and k_dropout_fwd run this one function)
__host__ __device__ inline bool dropout_keep(unsigned long long stem, unsigned long long q, unsigned thr) {
    unsigned long long z = stem + (q + 1ull) * 0x9E3779B97F4A7C15ull;
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    z ^= z >> 31;
    return (unsigned)(z >> 40) >= thr;
}

struct DropSpec {
    unsigned long long seed;
    unsigned long long site48;    // (uint64)d << 48
    unsigned thr;
    float s;
};

__global__ void k_dropout_tick(long long* t) {
    if (blockIdx.x == 0 && threadIdx.x == 0) *t = *t + 1;
}

// a: [B][U] fp32, 16-byte aligned, U % 4 == 0; n4 = B * U / 4
__global__ __launch_bounds__(kDropThreads) void k_dropout_fwd(float* __restrict__ a, long long n4, int U, DropSpec d, const long long* __restrict__ t_dev, long long t_imm) {
#pragma clang fp contract(off)
    const long long i = (long long)blockIdx.x * kDropThreads + threadIdx.x;
    if (i >= n4) return;
    const unsigned long long stem = dropout_stem(d.seed, (unsigned long long)(t_dev ? *t_dev : t_imm));
    const long long idx = i * 4;
    const long long r = idx / U;
    const unsigned long long row = d.site48 + (unsigned long long)(r * U);      // the four units of this thread lie in one row
    const unsigned long long u = (unsigned long long)(idx - r * U);
    f32x4* const p = reinterpret_cast<f32x4*>(a + idx);
    f32x4 v = *p;
#pragma unroll
    for (int k = 0; k < 4; ++k) v[k] = dropout_keep(stem, row + u + (unsigned long long)k, d.thr) ? v[k] * d.s : 0.0f;
    *p = v;
}

// g: [B][U] fp32, 16-byte aligned; n4 = B * U / 4
__global__ __launch_bounds__(kDropThreads) void k_dropout_bwd(float* __restrict__ g, long long n4, float s) {
#pragma clang fp contract(off)
    const long long i = (long long)blockIdx.x * kDropThreads + threadIdx.x;
    if (i >= n4) return;
    f32x4* const p = reinterpret_cast<f32x4*>(g + i * 4);
    *p = *p * s;
}

}  // namespace rcnx
