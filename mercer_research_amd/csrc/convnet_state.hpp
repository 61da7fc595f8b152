// convnet_state.hpp -- Track X: the whole training state of a net packed into ONE contiguous device buffer and back (rcn_hipx_snapshot_dev,
// rcn_hipx_restore_dev).  No reference counterpart.
//
// The body, a 16-byte aligned device buffer the caller owns:
//     [0, 256)            the scalars block: raw copies of the 32-byte AdamTick (convnet_adam.hpp) at byte 0, the 8-byte dropout ordinal
//                         (convnet_dropout.hpp) at byte 32 and the 16-byte clip state [counter][norm][coef] (convnet_clip.hpp) at byte 40;
//                         a buffer the net does not have, and bytes 56 .. 255, are zero
//     sec[s].body_off     section s -- parameters, velocity, Adam m, Adam v, average, accumulator, those that are selected -- in the LOGICAL
//                         layout of rcn_hipx_get_params: per layer W[K][Cout] then b[Cout], all layers back to back; every section starts
//                         at a multiple of 256 bytes, and the bytes between its end and the next such multiple are zero
// The net's side is the padded layout: per layer [W | b] as (K + 1) rows of CoutP floats, layers back to back without a gap.
//
// Both kernels are pure copies: no arithmetic, no LDS, no atomics.  The work of one section is cut into units of kStateUnit elements of one
// layer, the layer table (StateJobs, by value like the reduction's ReduceJobs) saying which unit belongs to which layer; a workgroup takes
// units blockIdx.x, + gridDim.x, ... of all sections in turn, so ONE launch covers everything.  A layer with Cout == CoutP whose two offsets
// are multiples of four floats (every layer but a logits layer with padded class columns) moves as 16-byte pieces; any other element by
// element with a division per element.
//
//   k_state_pack     padded -> logical.  Reads the net, writes only the body.
//   k_state_unpack   logical -> padded.  Writes EVERY element of a restored buffer: the logical value, or +0.0f for a padding column, so
//                    p = e = 0 on padding holds afterwards whatever the buffer held (the update kernels rely on it).  Writes back those
//                    scalar blocks whose pointer is set.
#pragma once

#include "convnet.hpp"

namespace rcnx {

constexpr int kStateSections = 6;           // parameters, velocity, Adam m, Adam v, average, accumulator: bit s of a section mask
constexpr int kStateScalarsBytes = 256;     // the scalars block; the three copies sit at these byte offsets
constexpr int kStateTickAt = 0, kStateTickBytes = 32, kStateDropAt = 32, kStateDropBytes = 8, kStateClipAt = 40, kStateClipBytes = 16;
constexpr int kStateMaxJobs = 32;           // layers with parameters (the reduction launch takes as many: kMaxReduceJobs)
constexpr int kStateThreads = 256;
constexpr int kStateUnit = 4096;            // elements of one layer per workgroup and trip: 256 threads x four 16-byte pieces
constexpr int kStateMaxBlocks = 2048;       // the grid's cap; the units beyond it are reached by the stride

struct StateJob {
    long long pad_off, log_off;             // the layer's [W | b] in the padded and in the logical layout, in floats
    long long n_pad, n_log;                 // (K + 1) * CoutP and (K + 1) * Cout
    int Cout, CoutP;
    int vec;                                // 16-byte pieces
    int first_unit;                         // pack: of n_log elements; unpack: of n_pad elements
};
struct StateSection { float* pad; long long body_off; };      // the net's padded buffer and the section's place in the body, in floats
struct StateJobs {
    StateJob j[kStateMaxJobs];
    StateSection sec[kStateSections];
    int njobs, nsec, units;                 // units of ONE section (every section has the same layer table)
    long long n_log; int gap;               // a section's floats, and the floats from there to the next multiple of 256 bytes (< 64): pack zeroes them
    unsigned* tick; unsigned* drop; unsigned* clip;      // the net's three scalar buffers as 4-byte words (nullptr: the net has none / not restored)
};

inline int state_units(long long n) { return (int)((n + kStateUnit - 1) / kStateUnit); }

// the layer a unit belongs to (at most kStateMaxJobs = 32 jobs: a scan)
__device__ __forceinline__ int state_job_of(const StateJobs& J, int unit) {
    int q = 0;
    while (q + 1 < J.njobs && unit >= J.j[q + 1].first_unit) ++q;
    return q;
}

__global__ __launch_bounds__(kStateThreads) void k_state_pack(StateJobs J, float* __restrict__ body) {
    if (blockIdx.x == 0 && threadIdx.x < kStateScalarsBytes / 4) {
        const int w = threadIdx.x;
        unsigned v = 0;
        if (w < kStateDropAt / 4) { if (J.tick) v = J.tick[w]; }
        else if (w < kStateClipAt / 4) { if (J.drop) v = J.drop[w - kStateDropAt / 4]; }
        else if (w < (kStateClipAt + kStateClipBytes) / 4) { if (J.clip) v = J.clip[w - kStateClipAt / 4]; }
        reinterpret_cast<unsigned*>(body)[w] = v;
        if (w < J.gap)
            for (int s = 0; s < J.nsec; ++s) body[J.sec[s].body_off + J.n_log + w] = 0.0f;      // a body has no byte the launch leaves undefined
    }
    const long long total = (long long)J.nsec * J.units;
    for (long long u = blockIdx.x; u < total; u += gridDim.x) {
        const int s = (int)(u / J.units), unit = (int)(u - (long long)s * J.units);
        const StateJob jb = J.j[state_job_of(J, unit)];
        const float* __restrict__ src = J.sec[s].pad + jb.pad_off;
        float* __restrict__ dst = body + J.sec[s].body_off + jb.log_off;
        const long long base = (long long)(unit - jb.first_unit) * kStateUnit;
        if (jb.vec) {
#pragma unroll
            for (int k = 0; k < kStateUnit / (4 * kStateThreads); ++k) {
                const long long i = base + ((long long)k * kStateThreads + threadIdx.x) * 4;      // n_log % 4 == 0 (host)
                if (i < jb.n_log) *reinterpret_cast<f32x4*>(dst + i) = *reinterpret_cast<const f32x4*>(src + i);
            }
        } else {
            for (int k = 0; k < kStateUnit / kStateThreads; ++k) {
                const long long i = base + (long long)k * kStateThreads + threadIdx.x;
                if (i < jb.n_log) { const long long r = i / jb.Cout; dst[i] = src[r * jb.CoutP + (i - r * jb.Cout)]; }
            }
        }
    }
}

__global__ __launch_bounds__(kStateThreads) void k_state_unpack(StateJobs J, const float* __restrict__ body) {
    if (blockIdx.x == 0 && threadIdx.x < (kStateClipAt + kStateClipBytes) / 4) {
        const int w = threadIdx.x;
        const unsigned v = reinterpret_cast<const unsigned*>(body)[w];
        if (w < kStateDropAt / 4) { if (J.tick) J.tick[w] = v; }
        else if (w < kStateClipAt / 4) { if (J.drop) J.drop[w - kStateDropAt / 4] = v; }
        else if (J.clip) J.clip[w - kStateClipAt / 4] = v;
    }
    const long long total = (long long)J.nsec * J.units;
    for (long long u = blockIdx.x; u < total; u += gridDim.x) {
        const int s = (int)(u / J.units), unit = (int)(u - (long long)s * J.units);
        const StateJob jb = J.j[state_job_of(J, unit)];
        const float* __restrict__ src = body + J.sec[s].body_off + jb.log_off;
        float* __restrict__ dst = J.sec[s].pad + jb.pad_off;
        const long long base = (long long)(unit - jb.first_unit) * kStateUnit;
        if (jb.vec) {
#pragma unroll
            for (int k = 0; k < kStateUnit / (4 * kStateThreads); ++k) {
                const long long i = base + ((long long)k * kStateThreads + threadIdx.x) * 4;      // n_pad == n_log, % 4 == 0 (host)
                if (i < jb.n_pad) *reinterpret_cast<f32x4*>(dst + i) = *reinterpret_cast<const f32x4*>(src + i);
            }
        } else {
            for (int k = 0; k < kStateUnit / kStateThreads; ++k) {
                const long long i = base + (long long)k * kStateThreads + threadIdx.x;
                if (i < jb.n_pad) { const long long r = i / jb.CoutP; const int c = (int)(i - r * jb.CoutP); dst[i] = c < jb.Cout ? src[r * jb.Cout + c] : 0.0f; }
            }
        }
    }
}

}  // namespace rcnx
