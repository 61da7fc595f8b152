// convnet_gap.hpp -- Track X: global average pooling in front of the dense stage (RCN_HIPX_GLOBAL_AVGPOOL), torch.nn.AdaptiveAvgPool2d(1)
// followed by flatten(1) over an NHWC fp32 map x[B][HW][C], HW = H * W rows per sample, C % 32 == 0:
//     y[b][c] = mean over r of x[b][r][c]
// Two streaming kernels, 16-byte accesses, no atomics of any kind.
//
// k_gap_fwd   workgroup (b, j) of a (B, gap_col_blocks(C)) grid takes sample b and the float4 columns [64 j, 64 j + cols), cols <= 64.  Its 256
//             threads are cols x slices, slices = gap_slices(cols) = 256 / cols rounded down (threads past cols * slices idle: C = 96 is
//             24 x 10).  Thread (slice, col) adds the rows slice, slice + slices, ... of its four channels in ascending order, four loads
//             in flight; the first `cols` threads add the slices in the order 0 .. slices - 1 through LDS and write the mean.  A slice
//             without a row (HW < slices) is not read by the combine: it contributes nothing.
//             The sums are made in DOUBLE, as batch normalisation's are (convnet_bn.hpp): every term is exact, a map of a few thousand rows
//             loses nothing to the order of the additions, and the kernel is bound by its loads either way.  The mean is ONE true division
//             in double, rounded to float once: y = fl32(S / (double)HW).
//             One sample per workgroup and no loop over samples: the layout of the sum is a function of (HW, C) alone -- never of B, of the
//             grid or of which workgroup finishes first -- so every output has ONE order per shape.
// k_gap_bwd   din[b][r][c] = (GATE && !(out_below[b][r][c] > 0)) ? 0 : fl(g[b][c] / (float)HW), g the layer's dout as the dense layer above
//             wrote it (ungated: the pool has no ReLU of its own).  One thread per four channels, grid-stride with the cap of the batch
//             normalisation streaming kernels (bn_stream_blocks: a thread's four channels never change along its loop); the division is a
//             true fp32 division per element, so the result does not depend on which trip of which thread makes it.  GATE: the layer
//             below is a ReLU layer (a RCN_HIPX_CONV3X3_RELU or a batch normalisation of either kind) and finds its dZ ready; out_below is
//             read only then.  A max-pool below gates in its own backward pass.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "convnet.hpp"
#include "convnet_bn.hpp"

namespace rcnx {

constexpr int kGapThreads = 256;
constexpr int kGapCols = 64;                // float4 columns of one workgroup at most: 256 channels

// grid.y of k_gap_fwd, the columns of workgroup j and the row slices of a workgroup of `cols` columns: shape alone
__host__ __device__ inline int gap_col_blocks(int C) { return (C / 4 + kGapCols - 1) / kGapCols; }
__host__ __device__ inline int gap_cols(int C, int j) { const int left = C / 4 - j * kGapCols; return left < kGapCols ? left : kGapCols; }
__host__ __device__ inline int gap_slices(int cols) { return kGapThreads / cols; }

__global__ __launch_bounds__(kGapThreads) void k_gap_fwd(const float* __restrict__ x, float* __restrict__ y, int HW, int C) {
    __shared__ double red[kGapThreads][4];
    const int cols = gap_cols(C, (int)blockIdx.y), slices = gap_slices(cols);
    const int slice = (int)threadIdx.x / cols, col = (int)threadIdx.x % cols;
    const int c = ((int)blockIdx.y * kGapCols + col) * 4;
    const float* const xb = x + (long long)blockIdx.x * HW * C + c;
    double s[4] = {0, 0, 0, 0};
    if (slice < slices) {
        int r = slice;
        for (; r + 3 * slices < HW; r += 4 * slices) {
            f32x4 v[4];
#pragma unroll
            for (int u = 0; u < 4; ++u) v[u] = bn_load4(xb + (long long)(r + u * slices) * C);
#pragma unroll
            for (int u = 0; u < 4; ++u)
#pragma unroll
                for (int k = 0; k < 4; ++k) s[k] += (double)v[u][k];
        }
        for (; r < HW; r += slices) {
            const f32x4 v = bn_load4(xb + (long long)r * C);
#pragma unroll
            for (int k = 0; k < 4; ++k) s[k] += (double)v[k];
        }
    }
#pragma unroll
    for (int k = 0; k < 4; ++k) red[threadIdx.x][k] = s[k];
    __syncthreads();
    if (slice == 0) {
        const int used = HW < slices ? HW : slices;                  // (the slices past `used` hold no row)
        for (int j = 1; j < used; ++j)
#pragma unroll
            for (int k = 0; k < 4; ++k) s[k] += red[j * cols + col][k];
        f32x4 m;
#pragma unroll
        for (int k = 0; k < 4; ++k) m[k] = (float)(s[k] / (double)HW);
        *reinterpret_cast<f32x4*>(y + (long long)blockIdx.x * C + c) = m;
    }
}

template <bool GATE>
__global__ __launch_bounds__(kBnThreads) void k_gap_bwd(const float* __restrict__ g, const float* __restrict__ out_below, float* __restrict__ din, long long n4, int HW, int C) {
    const int C4 = C / 4;
    long long e = (long long)blockIdx.x * kBnThreads + threadIdx.x;
    if (e >= n4) return;
    const int c = (int)(e % C4) * 4;                                 // (the grid's threads are a multiple of C4: bn_stream_blocks)
    // the row of the thread's piece as (sample, row of the sample), advanced by the grid's stride without a division per trip
    const long long stride_rows = (long long)gridDim.x * kBnThreads / C4;
    const long long step_b = stride_rows / HW;
    const int step_r = (int)(stride_rows % HW);
    long long b = e / C4 / HW;
    int r = (int)(e / C4 % HW);
    const float hw = (float)HW;
    for (; e < n4; e += (long long)gridDim.x * kBnThreads) {
        const f32x4 gv = bn_load4(g + b * C + c);
        f32x4 v;
#pragma unroll
        for (int k = 0; k < 4; ++k) v[k] = gv[k] / hw;
        if (GATE) {
            const f32x4 yv = bn_load4(out_below + e * 4);
#pragma unroll
            for (int k = 0; k < 4; ++k) v[k] = yv[k] > 0.f ? v[k] : 0.f;
        }
        *reinterpret_cast<f32x4*>(din + e * 4) = v;
        b += step_b; r += step_r;
        if (r >= HW) { r -= HW; ++b; }
    }
}

}  // namespace rcnx
