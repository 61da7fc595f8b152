// convnet_accum.hpp -- Track X: gradient accumulation over micro-batches (rcn_hipx_set_accumulate), what torch users write as
// (loss / k).backward() k times, then clip_grad_norm_, opt.step() and zero_grad().  No reference counterpart.
//
// With c = fl(1.0f / k) computed once on the host and g_j the summed gradient of micro-batch j in the padded flat layout (the value
// rcn_hipx_gradients_dev returns for that batch, bit for bit).  fp32, every operation rounded once (no fused multiply-add):
//     acc = fl(c * g_0)                   the first micro-step of a cycle: a store, so nothing needs zeroing
//     acc = fl(acc + fl(c * g_j))         micro-steps j = 1 .. k - 1, in order
// After micro-step k - 1 acc IS the step's gradient: the host hands every layer's slice of it to the net's update launch as a one-chunk
// slab (k_grad_sumsq in front of it where clipping is on), exactly as the clipped step hands over its gradient buffer, so the flipped
// weight copy, the velocity, the average and the clip state are kept by the launches that have always kept them.  The scale goes in per
// micro-batch, not at the end: acc then never holds more than one batch's magnitude, and a cycle cut short holds a mean, not a sum.
// tests/_accum_ref.py restates it in NumPy, bit for bit.
//
//   Accumulate<FIRST>    an update functor of reduce_all_body whose "parameters" are acc: the job table's p points at the layer's slice
//                        of acc and has neither a gradient destination nor a flipped copy
//   k_reduce_all_acc<FIRST>
//                        the step's ONE slab reduction of a micro-step: the grid, the 16-byte accesses and the fixed summation order of
//                        the update launch (k_reduce_update); FIRST stores fl(c * t), the other form reads acc and adds
#pragma once

#include "convnet.hpp"

namespace rcnx {

template <bool FIRST> struct Accumulate {
    float c;
    __device__ __forceinline__ f32x4 operator()(const ReduceJobs&, const ReduceJob& jb, long long i, const f32x4& t) const {
#pragma clang fp contract(off)
        const f32x4 s = c * t;
        if constexpr (FIRST) return s;
        else return *reinterpret_cast<const f32x4*>(jb.p + i) + s;
    }
};

template <bool FIRST>
__global__ __launch_bounds__(kReduceThreads) void k_reduce_all_acc(ReduceJobs J, float c) { reduce_all_body(J, Accumulate<FIRST>{c}); }

}  // namespace rcnx
