// convnet_update.hpp -- Track X: the step's update launch, ONE kernel template over the four things a net may configure: clipping
// (convnet_clip.hpp), the optimiser (convnet_sgd.hpp, convnet_adam.hpp), the average (convnet_ema.hpp) and a rate read from a device
// scalar (convnet.hpp).
//
//   k_reduce_update<CLIP, OPT, EMA, DLR>
//       reduce_all_body with the functor Clipped<WithEma<DeviceLr<PlainUpdate | SgdUpdate | AdamUpdate>>>, every wrapper present only where
//       its flag is set; OPT is kOptPlain, kOptSgd or kOptAdam.  The nesting is fixed: the rate is replaced innermost, the average sees the
//       parameters the update stores, the coefficient multiplies the gradient before anything else reads it.  PlainUpdate and SgdUpdate
//       stay separate instantiations: they round differently (convnet_clip.hpp).  clip_coef_all is called by every workgroup, before the body.
//       <false, kOptPlain, false, false> with J.apply == 0 is the gradients-only walk.
//
// The plan (rcn_hipx_plan...) prints an instantiation as k_reduce_all[_clip][_sgd | _adam][_ema][_dlr]: that is its display name
// (describe_update, convnet_select.hpp), one suffix per flag that is set.
#pragma once

#include <type_traits>

#include "convnet_adam.hpp"

namespace rcnx {

// the innermost functor of k_reduce_update: p - lr g, rcn_hipx_set_sgd's update, rcn_hipx_set_adam's
constexpr int kOptPlain = 0, kOptSgd = 1, kOptAdam = 2;

// A form's argument list holds what its flags name and nothing else, in the order (and so at the kernarg offsets) of the named kernels'
// parameter lists: SgdParams (or AdamParams: the optimiser's slot), EmaParams, ClipParams, the rate's device scalar.  One struct of all four behind ReduceJobs compiled to the
// same code with a 1152-byte kernarg segment in every form; both are measured against the named kernels in
// profiles/trackx_update_refactor_ab.txt (the struct further from them, these lists closer, three configurations not inside their range).
template <bool ON, class T, int SLOT> struct ArgIf { T v; };
template <class T, int SLOT> struct ArgIf<false, T, SLOT> {};
template <int OPT> using OptParams = std::conditional_t<OPT == kOptAdam, AdamParams, SgdParams>;
template <bool CLIP, int OPT, bool EMA, bool DLR>
struct UpdateArgs : ArgIf<OPT != kOptPlain, OptParams<OPT>, 0>, ArgIf<EMA, EmaParams, 1>, ArgIf<CLIP, ClipParams, 2>, ArgIf<DLR, const float*, 3> {
    __host__ __device__ OptParams<OPT>& opt() { return ArgIf<OPT != kOptPlain, OptParams<OPT>, 0>::v; }      // SgdParams or AdamParams, by OPT
    __host__ __device__ EmaParams& ema() { return ArgIf<EMA, EmaParams, 1>::v; }
    __host__ __device__ ClipParams& clip() { return ArgIf<CLIP, ClipParams, 2>::v; }
    __host__ __device__ const float*& lr() { return ArgIf<DLR, const float*, 3>::v; }      // the step's rate, a device scalar
};

// Neither J nor A is written: a written kernel argument that is indexed at run time is copied to scratch (DeviceLr, convnet.hpp)
template <bool CLIP, int OPT, bool EMA, bool DLR>
__global__ __launch_bounds__(kReduceThreads) void k_reduce_update(ReduceJobs J, UpdateArgs<CLIP, OPT, EMA, DLR> A) {
    // the functor in plain locals, innermost first (built through lambdas or helpers the SGD forms compile to other code than the named kernels did)
    using Base = std::conditional_t<OPT == kOptAdam, AdamUpdate, std::conditional_t<OPT == kOptSgd, SgdUpdate, PlainUpdate>>;
    using Rated = std::conditional_t<DLR, DeviceLr<Base>, Base>;
    using Averaged = std::conditional_t<EMA, WithEma<Rated>, Rated>;
    Base base{};
    if constexpr (OPT == kOptSgd) base.s = A.opt();
    if constexpr (OPT == kOptAdam) base.a = A.opt();
    Rated rated{};
    if constexpr (DLR) { rated.u = base; rated.lr = *A.lr(); } else rated = base;
    Averaged averaged{};
    if constexpr (EMA) { averaged.u = rated; averaged.m = A.ema(); } else averaged = rated;
    if constexpr (CLIP) reduce_all_body(J, Clipped<Averaged>{averaged, clip_coef_all(A.clip())});
    else reduce_all_body(J, averaged);
}

}  // namespace rcnx
