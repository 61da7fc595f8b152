// convnet_epoch.hpp -- Track X: the loop around the training step (rcn_hipx_train_epoch_dev / _ex_dev, rcn_hipx_gather_batch_dev,
// rcn_hipx_evaluate_dev).  No reference counterpart; the main track's counterparts are rcn_hip_shuffle_dev / rcn_hip_evaluate*.
//
//   k_gather_rows<TS, VEC>  rows of a device-resident set (fp32 or uint8), selected by an int32 index row, into the net's contiguous
//                           fp32 batch buffer, and their labels into its int32 labels buffer.  Every index is clamped into [0, n)
//                           before it forms an address.
//   k_gather_aug<TS, VEC>   the same rows through a random translation with zero padding and a horizontal flip (rcn_hipx_augment): the
//                           sample's draw is computed from its position in the epoch in registers; element by element on the read side,
//                           16-byte stores on the write side.
//   k_gather_mix<TS, VEC>   mixup / CutMix (rcn_hipx_mix_step): every output row blended with, or inside a box replaced by, the row that
//                           mirrors it in the SAME batch, each gathered (and augmented) as the kernels above would; both labels out.
// The evaluation kernel behind rcn_hipx_evaluate_dev is k_eval<false> (convnet_metrics.hpp).
#pragma once

#include <type_traits>

#include "convnet.hpp"

namespace rcnx {

using u32x4 = __attribute__((ext_vector_type(4))) unsigned;

// how the values of a resident set become the fp32 values the net reads (RCN_HIPX_X_U8: two roundings, no fused multiply-add)
struct RowScale { float scale, shift; };

template <typename TS> struct RowPiece;
// 16 bytes of an fp32 row: four values, copied
template <> struct RowPiece<float> {
    static constexpr int kVec = 4;
    using type = f32x4;
    __device__ static inline void store(float* __restrict__ dst, const f32x4& v, const RowScale&) { *reinterpret_cast<f32x4*>(dst) = v; }
    __device__ static inline float widen1(float v, const RowScale&) { return v; }
};
// 16 bytes of a uint8 row: sixteen values, widened in registers, stored as four 16-byte pieces
template <> struct RowPiece<uint8_t> {
    static constexpr int kVec = 16;
    using type = u32x4;
    __device__ static inline float widen1(uint8_t v, const RowScale& rs) {
#pragma clang fp contract(off)
        const float m = (float)v * rs.scale;
        return m + rs.shift;
    }
    __device__ static inline void store(float* __restrict__ dst, const u32x4& v, const RowScale& rs) {
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            f32x4 o;
#pragma unroll
            for (int b = 0; b < 4; ++b) o[b] = widen1((uint8_t)((v[q] >> (8 * b)) & 0xffu), rs);
            *reinterpret_cast<f32x4*>(dst + 4 * q) = o;
        }
    }
};

constexpr int kGatherSlots = 4;        // 64-lane pieces a wave has in flight: four short rows at once, or 4 KiB of a long one
constexpr int kGatherThreads = 256;

// dst[r][0 .. E) = widen(X[row(r)][0 .. E)) and labels_out[r] = labels[row(r)] for r < B, where row(r) = clamp(idx ? idx[r] : base + r, 0, n - 1).
// One wave takes kGatherSlots consecutive slots of the flattened (destination row, 64-piece slot) space: rows shorter than a wave's 64
// pieces (MNIST as uint8: 49 pieces of 16 bytes) travel four to a wave, long rows (CIFAR as fp32: 768 pieces) are cut into runs of
// 4 KiB; either way every load of the wave is issued before its first store.  VEC = RowPiece<TS>::kVec: 16-byte loads and stores (the host
// checks E % VEC == 0 and the bases' alignment); VEC = 1: element by element, for rows whose length or base does not allow them.
template <typename TS, int VEC>
__global__ __launch_bounds__(kGatherThreads) void k_gather_rows(const TS* __restrict__ X, const int* __restrict__ labels, long long n, const int* __restrict__ idx, long long base,
                                                                int B, int E, RowScale rs, float* __restrict__ dst, int* __restrict__ labels_out) {
    using Piece = typename std::conditional<VEC == 1, TS, typename RowPiece<TS>::type>::type;
    const int lane = threadIdx.x & 63;
    const unsigned wave = blockIdx.x * (kGatherThreads / 64) + (threadIdx.x >> 6);
    const int P = E / VEC;                              // pieces per row
    const unsigned S = (unsigned)(P + 63) / 64;         // slots per row
    const unsigned total = (unsigned)B * S;             // (B * S < 2^31: gather_blocks checks it)
    Piece v[kGatherSlots];
    long long at[kGatherSlots];                         // destination element offset; -1: nothing to do
#pragma unroll
    for (int j = 0; j < kGatherSlots; ++j) {
        const unsigned g = wave * kGatherSlots + j;
        at[j] = -1;
        if (g >= total) continue;
        const int r = (int)(g / S);
        const int piece = (int)(g % S) * 64 + lane;
        long long row = idx ? (long long)idx[r] : base + r;
        row = row < 0 ? 0 : (row >= n ? n - 1 : row);   // an index out of range is a caller error; it must not become an address
        if (labels && piece == 0) labels_out[r] = labels[row];
        if (piece >= P) continue;
        v[j] = *reinterpret_cast<const Piece*>(X + row * E + (long long)piece * VEC);
        at[j] = (long long)r * E + (long long)piece * VEC;
    }
#pragma unroll
    for (int j = 0; j < kGatherSlots; ++j) {
        if (at[j] < 0) continue;
        if constexpr (VEC == 1) dst[at[j]] = RowPiece<TS>::widen1(v[j], rs);
        else RowPiece<TS>::store(dst + at[j], v[j], rs);
    }
}

// workgroups of k_gather_rows for a batch of B rows of E elements; 0: more slots than the kernel's 32-bit slot index counts
inline long long gather_blocks(int B, int E, int vec) {
    const long long S = (E / vec + 63) / 64, waves = ((long long)B * S + kGatherSlots - 1) / kGatherSlots;
    if ((long long)B * S >= (1ll << 31) - kGatherSlots * (kGatherThreads / 64)) return 0;
    return (waves + kGatherThreads / 64 - 1) / (kGatherThreads / 64);
}

// ---- augmentation: random crop with zero padding, horizontal flip (rcn_hipx_augment) ---------------------------------------------------
struct AugSpec { unsigned long long seed, epoch; int pad, hflip; };
struct AugDraw { int dy, dx, flip; };

// The draw of the sample at absolute position q of the epoch: one splitmix64 output of a counter, nothing kept in memory, so the kernel
// and rcn_hipx_augment_draw (host) share this one function and splitting an epoch into calls changes nothing.  All arithmetic wraps in
// uint64.  dy and dx take 16 bits each through a multiply-shift, (bits * (2 pad + 1)) >> 16: of the 65536 inputs each of the 2 pad + 1
// outcomes gets floor or ceil of 65536 / (2 pad + 1), so an outcome's probability is off by less than 1 / 65536 and the ratio of two
// outcomes' probabilities by less than (2 pad + 1) / 65536 (pad <= 16: 5e-4).  flip is bit 32.
__host__ __device__ inline AugDraw augment_draw(const AugSpec& a, unsigned long long q) {
    unsigned long long z = a.seed ^ (a.epoch * 0xD1342543DE82EF95ull);
    z += (q + 1) * 0x9E3779B97F4A7C15ull;
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    z ^= z >> 31;
    const unsigned span = 2u * (unsigned)a.pad + 1u;
    AugDraw d;
    d.dy = (int)((((unsigned)z & 0xffffu) * span) >> 16) - a.pad;
    d.dx = (int)((((unsigned)(z >> 16) & 0xffffu) * span) >> 16) - a.pad;
    d.flip = a.hflip ? (int)((z >> 32) & 1u) : 0;
    return d;
}

// dst[r][h][w][c] = widen(S(h + dy, (flip ? W - 1 - w : w) + dx, c)) for r < B, where S is the stored value of row(r) of the set -- the
// stored value 0 outside the image -- (dy, dx, flip) = augment_draw(aug, q0 + r) and row(r) is k_gather_rows' clamped row; labels as there.
// This is a crop of the image padded with `pad` zeros on every side, then a mirror (torchvision: RandomCrop(padding = pad), then
// RandomHorizontalFlip).  One thread per VEC consecutive outputs of a row (VEC = 4: one 16-byte store, the host checks E % 4 == 0 and the
// destination's alignment; VEC = 1 otherwise): for each it decodes (h, w, c), loads ONE source element -- a shifted, mirrored NHWC row of 1
// or 3 channels has no 16-byte pieces to move -- or takes the stored 0, and widens it.  The write side (4 bytes per element, 4x the read
// side of a uint8 set) is fully coalesced; the source batch is a few MB read once.  No address is formed from a coordinate outside the
// image.  total = B * (E / VEC) threads (gather_aug_blocks).
template <typename TS, int VEC>
__global__ __launch_bounds__(kGatherThreads) void k_gather_aug(const TS* __restrict__ X, const int* __restrict__ labels, long long n, const int* __restrict__ idx, long long base,
                                                               int B, int H, int W, int C, RowScale rs, AugSpec aug, unsigned long long q0, float* __restrict__ dst,
                                                               int* __restrict__ labels_out) {
    const int E = H * W * C, P = E / VEC;               // pieces per row
    const long long g = (long long)blockIdx.x * kGatherThreads + threadIdx.x;
    if (g >= (long long)B * P) return;
    const int r = (int)(g / P), piece = (int)(g - (long long)r * P);
    long long row = idx ? (long long)idx[r] : base + r;
    row = row < 0 ? 0 : (row >= n ? n - 1 : row);       // as in k_gather_rows: an index out of range must not become an address
    if (labels && piece == 0) labels_out[r] = labels[row];
    const AugDraw d = augment_draw(aug, q0 + (unsigned long long)r);
    const TS* __restrict__ src = X + row * E;
    float o[VEC];
#pragma unroll
    for (int k = 0; k < VEC; ++k) {
        const int e = piece * VEC + k;
        const int hw = e / C, c = e - hw * C;
        const int h = hw / W, w = hw - h * W;
        const int sh = h + d.dy, sw = (d.flip ? W - 1 - w : w) + d.dx;
        TS v = (TS)0;
        if (sh >= 0 && sh < H && sw >= 0 && sw < W) v = src[(sh * W + sw) * C + c];
        o[k] = RowPiece<TS>::widen1(v, rs);
    }
    float* const out = dst + (long long)r * E + (long long)piece * VEC;
    if constexpr (VEC == 4) *reinterpret_cast<f32x4*>(out) = f32x4{o[0], o[1], o[2], o[3]};
    else out[0] = o[0];
}

// workgroups of k_gather_aug; 0: more than a 32-bit grid counts
inline long long gather_aug_blocks(int B, int E, int vec) {
    const long long blocks = ((long long)B * (E / vec) + kGatherThreads - 1) / kGatherThreads;
    return blocks >= (1ll << 31) ? 0 : blocks;
}

// ---- mixed samples: mixup and CutMix (rcn_hipx_mix_step) --------------------------------------------------------------------------------
struct MixStep { float blend, weight; int y0, y1, x0, x1; };      // rcn_hipx_mix_step, one per training step; the gather never reads `weight`

// the value k_gather_aug writes at (h, w, c) of a row drawn d -- k_gather_rows' value for the draw (0, 0, no flip)
template <typename TS>
__device__ inline float gathered_value(const TS* __restrict__ src, int h, int w, int c, int H, int W, int C, const AugDraw& d, const RowScale& rs) {
    const int sh = h + d.dy, sw = (d.flip ? W - 1 - w : w) + d.dx;
    TS v = (TS)0;
    if (sh >= 0 && sh < H && sw >= 0 && sw < W) v = src[(sh * W + sw) * C + c];
    return RowPiece<TS>::widen1(v, rs);
}

// Output row r of a batch of B mixed with its partner r' = B - 1 - r of the same batch (the middle row of an odd batch: itself).  With
// a = the value the un-mixed gather writes for row r at position q0 + r (k_gather_aug's if has_aug, else k_gather_rows') and b = the same
// for row r' at q0 + r' -- the counter-based draw makes the partner's augmentation free to recompute --
//     dst[r][h][w][c] = (mix->y0 <= h < mix->y1 && mix->x0 <= w < mix->x1) ? b              (CutMix's box, output coordinates, all channels)
//                     : mix->blend == 1 ? a : fl(fl(blend * a) + fl(fl(1 - blend) * b))     (mixup; no fused multiply-add)
//     labels_out[r] = label(row r), labels_b_out[r] = label(row r')                          (each nullable)
// *mix is ONE record on the device, never inspected: the box only chooses between two in-range sources, so any integers are safe, an
// inverted or outlying box included.  Indices are clamped as in the other gathers; no address is formed from a coordinate outside the
// image.  Only the sources an output needs are loaded (one inside the box or at blend 1, two where it blends).  Threads and stores as in
// k_gather_aug: one thread per VEC consecutive outputs, total = B * (E / VEC) (gather_aug_blocks).
template <typename TS, int VEC>
__global__ __launch_bounds__(kGatherThreads) void k_gather_mix(const TS* __restrict__ X, const int* __restrict__ labels, long long n, const int* __restrict__ idx, long long base,
                                                               int B, int H, int W, int C, RowScale rs, int has_aug, AugSpec aug, unsigned long long q0,
                                                               const MixStep* __restrict__ mix, float* __restrict__ dst, int* __restrict__ labels_out,
                                                               int* __restrict__ labels_b_out) {
    const int E = H * W * C, P = E / VEC;               // pieces per row
    const long long g = (long long)blockIdx.x * kGatherThreads + threadIdx.x;
    if (g >= (long long)B * P) return;
    const int r = (int)(g / P), piece = (int)(g - (long long)r * P), rp = B - 1 - r;
    long long row_a = idx ? (long long)idx[r] : base + r, row_b = idx ? (long long)idx[rp] : base + rp;
    row_a = row_a < 0 ? 0 : (row_a >= n ? n - 1 : row_a);      // as in k_gather_rows: an index out of range must not become an address
    row_b = row_b < 0 ? 0 : (row_b >= n ? n - 1 : row_b);
    if (labels && piece == 0) {
        if (labels_out) labels_out[r] = labels[row_a];
        if (labels_b_out) labels_b_out[r] = labels[row_b];
    }
    const MixStep m = *mix;
    const AugDraw none{0, 0, 0};
    const AugDraw da = has_aug ? augment_draw(aug, q0 + (unsigned long long)r) : none;
    const AugDraw db = has_aug ? augment_draw(aug, q0 + (unsigned long long)rp) : none;
    const TS* __restrict__ src_a = X + row_a * E;
    const TS* __restrict__ src_b = X + row_b * E;
    float o[VEC];
#pragma unroll
    for (int k = 0; k < VEC; ++k) {
        const int e = piece * VEC + k;
        const int hw = e / C, c = e - hw * C;
        const int h = hw / W, w = hw - h * W;
        if (h >= m.y0 && h < m.y1 && w >= m.x0 && w < m.x1) o[k] = gathered_value(src_b, h, w, c, H, W, C, db, rs);
        else if (m.blend == 1.0f) o[k] = gathered_value(src_a, h, w, c, H, W, C, da, rs);
        else {
#pragma clang fp contract(off)
            const float pa = m.blend * gathered_value(src_a, h, w, c, H, W, C, da, rs);
            const float pb = (1.0f - m.blend) * gathered_value(src_b, h, w, c, H, W, C, db, rs);
            o[k] = pa + pb;
        }
    }
    float* const out = dst + (long long)r * E + (long long)piece * VEC;
    if constexpr (VEC == 4) *reinterpret_cast<f32x4*>(out) = f32x4{o[0], o[1], o[2], o[3]};
    else out[0] = o[0];
}

// Which gather launch a batch gets.  Un-augmented: k_gather_rows, 16-byte pieces where every row starts on a 16-byte boundary and is a
// whole number of them, element by element otherwise.  Augmented: k_gather_aug, 16-byte stores where a row is a whole number of them.
// Mixed (augmented or not): k_gather_mix, by k_gather_aug's rule.
struct GatherChoice { bool aug, u8; int vec; long long blocks; bool mix = false; };
inline GatherChoice select_gather(bool u8, int B, int E, bool src_aligned16, bool dst_aligned16, bool aug, bool mix = false) {
    GatherChoice c{aug, u8, 1, 0, mix};
    if (aug || mix) {
        c.vec = (E % 4 == 0 && dst_aligned16) ? 4 : 1;
        c.blocks = gather_aug_blocks(B, E, c.vec);
        return c;
    }
    const int piece = u8 ? RowPiece<uint8_t>::kVec : RowPiece<float>::kVec;
    c.vec = (E % piece == 0 && src_aligned16 && dst_aligned16) ? piece : 1;
    c.blocks = gather_blocks(B, E, c.vec);
    return c;
}

}  // namespace rcnx
