// convnet_bf16.hpp -- Track X, the CDNA4 bf16 MFMA path (BASELINE.json configs[4] asks for one).
//
// Mixed precision in the usual sense: activations, gradients and parameters stay fp32 in HBM (master copies; the SGD update
// and every reduction are fp32), the two GEMM operands are rounded to bf16 (RNE, v_cvt_pk_bf16_f32) on their way into LDS,
// and v_mfma_f32_32x32x16_bf16 accumulates in fp32.  That is 8x the MFMA rate of the fp32 path (32x32x2) at the same
// HBM traffic, with ~2^-9 relative rounding per operand -- results agree with the f64 oracle to ~1e-2, which the tests
// state, not to the fp32 path's 1e-4.
//
// Operand layout (cdna_hip_programming.md, "A/B operand lane maps, bf16"): lane l (r = l & 31, h = l >> 5) holds
// A[row r][k = 8h + j] and B[k = 8h + j][col r], j = 0..7 -- eight CONSECUTIVE k per lane for both operands.  So both LDS
// tiles are stored k-contiguous and every fragment is one ds_read_b128:
//   A tile [128 rows][32 k]   rows of the implicit im2col matrix; thread loads 4 fp32 of a row (16 B), stores 4 bf16 (8 B)
//   B tile [BN cols][32 k]    from a bf16 copy of the weights stored TRANSPOSED, [Cout][K] (k_prep_weights_bf16, once per
//                             step and layer -- weights are small), so a tile row is a plain 64-byte run of HBM
// Row stride 40 halves (80 B): 16-byte aligned, and consecutive rows start 20 banks apart.
#pragma once

#include "convnet.hpp"

namespace rcnx {

using bf16x8 = __attribute__((ext_vector_type(8))) __bf16;

constexpr int kLdH = kBK + 8;      // halves per LDS tile row

// dst[c][r] = bf16(src[r][c]) for r < R, 0 for R <= r < Rp   (src: [R][C] fp32 row-major, dst: [C][Rp] bf16)
__global__ void k_prep_weights_bf16(const float* __restrict__ src, int R, int C, __bf16* __restrict__ dst, int Rp) {
    const long long total = (long long)C * Rp;
    for (long long e = (long long)blockIdx.x * blockDim.x + threadIdx.x; e < total; e += (long long)gridDim.x * blockDim.x) {
        const int c = (int)(e / Rp), r = (int)(e - (long long)c * Rp);
        dst[e] = r < R ? (__bf16)src[(long long)r * C + c] : (__bf16)0.f;
    }
}

// The same for every layer and both orientations in ONE launch at the start of a step (a launch per layer and pass was 5 us each, six of
// them on the CIFAR net: 9 % of the bf16 step).  The weights only change in the step's last kernel, so copies made at its start
// serve the forward and the backward pass.  Job q owns workgroups [first_block, next job's first_block), one 32 x 32 tile each.
constexpr int kMaxPrepJobs = 32;
struct PrepJob { const float* src; __bf16* dst; int R, C, Rp, first_block; };
struct PrepJobs { PrepJob j[kMaxPrepJobs]; int njobs; };
__host__ __device__ inline int prep_job_blocks(int C, int Rp) { return ((C + 31) / 32) * (Rp / 32); }      // 32 x 32 tiles (Rp is a multiple of 32)
__global__ __launch_bounds__(256) void k_prep_all_bf16(PrepJobs J) {
    // a workgroup transposes one 32 (r) x 32 (c) tile through LDS: rows of src read along c, rows of dst written along r -- both sides in
    // whole 64 / 128-byte pieces (element by element one side is strided: the 16 per-layer launches of the 224 x 224 net took 88 us, one
    // launch of the same loop 100)
    __shared__ float tile[32][33];
    int q = 0;
    while (q + 1 < J.njobs && (int)blockIdx.x >= J.j[q + 1].first_block) ++q;
    const PrepJob jb = J.j[q];
    const int lb = (int)blockIdx.x - jb.first_block, tiles_r = jb.Rp / 32;
    const int r0 = (lb % tiles_r) * 32, c0 = (lb / tiles_r) * 32;
    const int tx = threadIdx.x & 31, ty = threadIdx.x >> 5;
#pragma unroll
    for (int u = 0; u < 4; ++u) {
        const int r = r0 + ty + 8 * u, c = c0 + tx;
        tile[ty + 8 * u][tx] = (r < jb.R && c < jb.C) ? jb.src[(long long)r * jb.C + c] : 0.f;
    }
    __syncthreads();
#pragma unroll
    for (int u = 0; u < 4; ++u) {
        const int c = c0 + ty + 8 * u, r = r0 + tx;
        if (c < jb.C) jb.dst[(long long)c * jb.Rp + r] = (__bf16)tile[tx][ty + 8 * u];
    }
}

// Same tiling, split-K and epilogues as k_conv_fwd; WB = weights as bf16 [Cout][Kp], Kp = K rounded up to 32
// TX / TY: storage types of X and of Y (and of EPI 3's gate tensor, which arrives through `bias`); a split-K launch writes float partials
// SH: k_conv_fwd's three geometries (ConvShapeS2T: WB is the bf16 copy of the tap-flipped transposed weights)
template <int KS, bool SMALLC, int BN, int EPI, typename TX = float, typename TY = float, class SH = ConvShape>
__global__ __launch_bounds__(kThreads) void k_conv_fwd_bf16(const TX* __restrict__ X, const __bf16* __restrict__ WB,
                                                            const float* __restrict__ bias, TY* __restrict__ Y, SH s) {
    constexpr int NT = BN / 32;
    constexpr int BCH = (BN * 4 + kThreads - 1) / kThreads;          // 16-byte chunks of the B tile per thread
    __shared__ __attribute__((aligned(16))) __bf16 As[2][kBM * kLdH];
    __shared__ __attribute__((aligned(16))) __bf16 Bs[2][BN * kLdH];
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
    const long long M = gemm_rows(s);
    unsigned bx = blockIdx.x;
    int cls = 0;                                         // parity class (ConvShapeS2T): uniform over the workgroup
    if constexpr (kIsS2T<SH>) { const unsigned tpc = gridDim.x / 4; cls = parity_class_of_block(bx, tpc); bx %= tpc; }
    const long long m0 = (long long)bx * kBM;
    const int n0 = blockIdx.y * BN;
    const int K = KS * KS * s.Cin;
    const int Kp = (K + kBK - 1) / kBK * kBK;
    const int nkt_all = kIsS2T<SH> ? parity_taps(cls) * (s.Cin / kBK) : Kp / kBK;
    const int kt0 = (int)((long long)nkt_all * blockIdx.z / gridDim.z), kt1 = (int)((long long)nkt_all * (blockIdx.z + 1) / gridDim.z);
    const int nkt = kt1 - kt0;
    Y += (long long)blockIdx.z * M * s.Cout;

    f32x16 acc[NT];
#pragma unroll
    for (int t = 0; t < NT; ++t)
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[t][r] = 0.f;

    f32x4 av[4];
    bf16x8 bv[BCH];
    // K-tile kt: its first column of WB, and (parity classes) its tap's dZ pixel offset and first channel
    struct Tile { int k0, dh, dw, c0; };
    auto tile_of = [&](int kt) {
        if constexpr (kIsS2T<SH>) {
            const int cpt = s.Cin / kBK, lt = kt / cpt, c0 = (kt - lt * cpt) * kBK;
            const ParityTap pt = parity_tap(cls, lt);
            return Tile{pt.tap * s.Cin + c0, pt.dh, pt.dw, c0};
        } else return Tile{kt * kBK, 0, 0, 0};
    };
    auto load_a = [&](const ARows& rows, int kt) {
        if constexpr (kIsS2T<SH>) { const Tile t = tile_of(kt); load_a_tap(X, s.H / 2, s.W / 2, s.Cin, rows, t.dh, t.dw, t.c0 + (tid & 7) * 4, av); }
        else load_a_regs<KS, SMALLC, TX>(X, s, rows, kt, tid, av);
    };
    auto load_b = [&](int kt) {
        const int kfirst = tile_of(kt).k0;
#pragma unroll
        for (int q = 0; q < BCH; ++q) {
            const int e = tid + kThreads * q;
            const int ec = e < BN * 4 ? e : 0;                        // unconditional load from a clamped address
            const int col = ec >> 2, kq = ec & 3;
            bv[q] = *reinterpret_cast<const bf16x8*>(WB + (long long)(n0 + col) * Kp + kfirst + kq * 8);
        }
    };
    auto store_tiles = [&](int buf) {
        const int c4 = (tid & 7) * 4;
#pragma unroll
        for (int q = 0; q < 4; ++q)
            *reinterpret_cast<bf16x4*>(&As[buf][((tid >> 3) + 32 * q) * kLdH + c4]) = to_bf16x4(av[q]);
#pragma unroll
        for (int q = 0; q < BCH; ++q) {
            const int e = tid + kThreads * q;
            if (e < BN * 4) *reinterpret_cast<bf16x8*>(&Bs[buf][(e >> 2) * kLdH + (e & 3) * 8]) = bv[q];
        }
    };

    int* const orow_s = parity_row_table<kIsS2T<SH>>();      // parity classes: where each of the workgroup's 128 rows is written
    if constexpr (kIsS2T<SH>) { if (tid < kBM && m0 + tid < M) orow_s[tid] = (int)parity_out_row(s, cls, m0 + tid); }
    const ARows rows = decode_rows(s, M, m0, tid);
    load_a(rows, kt0);
    load_b(kt0);
    store_tiles(0);
    __syncthreads();
    for (int kt = 0; kt < nkt; ++kt) {
        const int cur = kt & 1;
        if (kt + 1 < nkt) {
            load_a(rows, kt0 + kt + 1);
            load_b(kt0 + kt + 1);
        }
        const __bf16* a = &As[cur][(wave * 32 + (lane & 31)) * kLdH + 8 * (lane >> 5)];
        const __bf16* b = &Bs[cur][(lane & 31) * kLdH + 8 * (lane >> 5)];
#pragma unroll
        for (int ks = 0; ks < kBK / 16; ++ks) {
            const bf16x8 af = *reinterpret_cast<const bf16x8*>(a + 16 * ks);
#pragma unroll
            for (int t = 0; t < NT; ++t) {
                const bf16x8 bf = *reinterpret_cast<const bf16x8*>(b + 32 * t * kLdH + 16 * ks);
                acc[t] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(af, bf, acc[t], 0, 0, 0);
            }
        }
        if (kt + 1 < nkt) {
            store_tiles(cur ^ 1);
            __syncthreads();
        }
    }
#pragma unroll
    for (int t = 0; t < NT; ++t) {
        const int co = n0 + 32 * t + (lane & 31);
        const float bb = (EPI == 1 || EPI == 2) ? bias[co] : 0.f;
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            long long m = m0 + wave * 32 + mfma32_row(lane, r);
            if (m < M) {
                if constexpr (kIsS2T<SH>) m = orow_s[wave * 32 + mfma32_row(lane, r)];      // the input pixel of this class's row
                float v = acc[t][r] + bb;
                if (EPI == 2) v = v > 0.f ? v : 0.f;
                if (EPI == 3) v = widen(reinterpret_cast<const TY*>(bias)[m * s.Cout + co]) > 0.f ? v : 0.f;      // dgrad: ReLU mask of the layer below, `bias` = its output
                Y[m * s.Cout + co] = narrow<TY>(v);
            }
        }
    }
}

using s16x4 = __attribute__((ext_vector_type(4))) short;

// ds_read_b64_tr_b16 (cdna_hip_programming.md T10): per 16-lane group a 4-row x 16-column block of 16-bit elements comes
// back column-major -- lane i of the group receives column i of the 4 rows.  Lane 4q+p supplies the address of row q,
// columns 4p..4p+3.  EXEC must be all ones; addresses 8-byte aligned.
__device__ inline s16x4 lds_read_tr16(const __bf16* p) {
    return __builtin_amdgcn_ds_read_tr16_b64_v4i16((__attribute__((address_space(3))) s16x4*)(p));
}

// One 32x32x16 operand fragment whose CONTRACTION index runs along the rows of a row-major LDS image: rows = pixels
// px0 .. px0+15, columns = col0 .. col0+31 (the operand's M or N index).  MFMA lane l (r = l & 31, h = l >> 5) needs rows
// px0 + 8h + j, j = 0..7, of column col0 + r: two transposed 4-row reads.
__device__ inline bf16x8 tr_fragment(const __bf16* img, int ld, int px0, int col0, int lane) {
    const int g = lane >> 4, i = lane & 15, q = i >> 2, p = i & 3;
    const __bf16* a = img + (px0 + 8 * (g >> 1) + q) * ld + col0 + 16 * (g & 1) + 4 * p;
    const s16x4 lo = lds_read_tr16(a), hi = lds_read_tr16(a + 4 * ld);
    union { s16x4 s[2]; bf16x8 v; } u;
    u.s[0] = lo; u.s[1] = hi;
    return u.v;
}

// dW partial tiles with bf16 operands: workgroup (kg, nb, chunk) of NKB waves computes rows [32 NKB kg, +32 NKB) x cols
// [BN nb, +BN) of dW over its pixel chunk -- wave w owns k-block NKB kg + w (a 32 x BN tile, no cross-wave reduction) --
// and writes slab[chunk][K + 1][Cout] exactly like k_conv_wgrad (row K = the chunk's bias gradient, summed in fp32 from
// the unrounded dZ values as they pass through registers).
//
// The contraction runs over PIXELS, which are the rows of both staged images (Xs[pixel][k], Ds[pixel][co], filled with
// plain 8-byte stores of converted fp32 rows); the MFMA wants 8 consecutive contraction indices per lane, i.e. a column of
// those images -- the hardware transposed read delivers exactly that, so no operand is ever transposed by software.
// A k-block lies inside one filter tap (Cin % 32 == 0), different waves' blocks may be different taps.
// TX: storage type of X (the first dense layer's input is the convolutional stage's last map)
// SH = ConvShapeS2: X gathered at the strided position, as in k_conv_wgrad (a strided layer's 9 Cin / 32 k-blocks are a multiple of three: NKB = 3)
template <int KS, int BN, int NKB, typename TX = float, class SH = ConvShape>
__global__ __launch_bounds__(64 * NKB) void k_conv_wgrad_bf16(const TX* __restrict__ X, const float* __restrict__ dZ,
                                                              float* __restrict__ slab, SH s, int pix_per_chunk, WgradGrid gd) {
    constexpr int NT = BN / 32, kPT = 128, NTHR = 64 * NKB;
    constexpr int LDX = 32 * NKB + 8, LDD = BN + 8;
    constexpr int XCH = kPT * 8 * NKB / NTHR;                              // f32x4 chunks of the X tile per thread (= 16)
    constexpr int DCH = (kPT * (BN / 4) + NTHR - 1) / NTHR;               // ... of the dZ tile
    __shared__ __attribute__((aligned(16))) __bf16 Xs[kPT * LDX];
    __shared__ __attribute__((aligned(16))) __bf16 Ds[kPT * LDD];
    __shared__ __attribute__((aligned(16))) float red[NTHR * 4];
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
    const long long M = gemm_rows(s);
    const int K = KS * KS * s.Cin, nkb = K / 32;
    int kgx, nby, chunk;
    if (!gd.decode((int)blockIdx.x, kgx, nby, chunk)) return;            // padding of the XCD-aware grid (uniform per workgroup)
    const int kb0 = kgx * NKB, n0 = nby * BN;
    const long long p0 = (long long)chunk * pix_per_chunk;
    const long long p1 = p0 + pix_per_chunk < M ? p0 + pix_per_chunk : M;

    f32x16 acc[NT];
#pragma unroll
    for (int t = 0; t < NT; ++t)
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[t][r] = 0.f;
    f32x4 colsum = {0.f, 0.f, 0.f, 0.f};

    // X loader: chunk e = tid + NTHR q -> pixel row e / (8 NKB), 4 floats at tile column 4 (e % (8 NKB)).  NTHR is a multiple
    // of 8 NKB, so a thread's tile column -- hence its k-block and filter tap -- is the same for all its chunks.
    const int xcol = (tid % (8 * NKB)) * 4;
    const int xkb = kb0 + xcol / 32;
    const bool xlive = xkb < nkb;
    const int k0 = (xlive ? xkb : 0) * 32, tap = k0 / s.Cin;
    const int dh = tap / KS - KS / 2, dw = tap % KS - KS / 2;
    const long long toff = ((long long)dh * s.W + dw) * s.Cin + (k0 - tap * s.Cin) + (xcol & 31);
    f32x4 xv[XCH], dv[DCH];
    const auto& so = out_map(s);                                           // the map PixelRow walks: the output's
    PixelRow<8> row((int)p0 + tid / (8 * NKB), so);                       // the thread's X rows: 8 pixels apart across q AND across stages (128 = 16 * 8)
    auto gload = [&](long long pb) {
#pragma unroll
        for (int q = 0; q < XCH; ++q) {
            const bool in = xlive && row.m < (int)p1;
            if constexpr (kIsS2<SH>) {
                // the taps are centred on input pixel (n, 2 oh, 2 ow), whose index is (n H + 2 oh) W + 2 ow = 4 m - 2 ow
                const bool ok = in && (unsigned)(2 * row.oh + dh) < (unsigned)s.H && (unsigned)(2 * row.ow + dw) < (unsigned)s.W;
                const f32x4 val = widen4(*reinterpret_cast<const chunk4_t<TX>*>(X + (ok ? (4LL * row.m - 2 * row.ow) * s.Cin + toff : 0)));
                xv[q] = ok ? val : f32x4{0, 0, 0, 0};
            } else {
                const bool ok = in && (unsigned)(row.oh + dh) < (unsigned)s.H && (unsigned)(row.ow + dw) < (unsigned)s.W;
                const f32x4 val = widen4(*reinterpret_cast<const chunk4_t<TX>*>(X + (ok ? (long long)row.m * s.Cin + toff : 0)));   // unconditional, masked by value
                xv[q] = ok ? val : f32x4{0, 0, 0, 0};
            }
            row.advance(so);
        }
#pragma unroll
        for (int q = 0; q < DCH; ++q) {
            const int e = tid + NTHR * q;
            const int ec = e < kPT * (BN / 4) ? e : 0;
            const int pr = ec / (BN / 4), c4b = (ec - pr * (BN / 4)) * 4;
            const long long m = pb + pr;
            const f32x4 val = *reinterpret_cast<const f32x4*>(dZ + (m < p1 ? m : p0) * s.Cout + n0 + c4b);
            dv[q] = (m < p1 && e < kPT * (BN / 4)) ? val : f32x4{0, 0, 0, 0};
        }
    };
    auto lstore = [&]() {
#pragma unroll
        for (int q = 0; q < XCH; ++q)
            *reinterpret_cast<bf16x4*>(&Xs[((tid + NTHR * q) / (8 * NKB)) * LDX + xcol]) = to_bf16x4(xv[q]);
#pragma unroll
        for (int q = 0; q < DCH; ++q) {
            const int e = tid + NTHR * q;
            if (e < kPT * (BN / 4)) {
                const int pr = e / (BN / 4), c4b = (e - pr * (BN / 4)) * 4;
                *reinterpret_cast<bf16x4*>(&Ds[pr * LDD + c4b]) = to_bf16x4(dv[q]);
                colsum += dv[q];                                             // fp32, unrounded: the bias gradient
            }
        }
    };

    const bool wlive = kb0 + wave < nkb;                                    // wave-uniform
    gload(p0);
    for (long long pb = p0; pb < p1; pb += kPT) {
        lstore();
        __syncthreads();
        if (pb + kPT < p1) gload(pb + kPT);                                 // next 128 pixels fly while these are contracted
        if (wlive) {
#pragma unroll
            for (int st = 0; st < kPT / 16; ++st) {
                const bf16x8 af = tr_fragment(Xs, LDX, 16 * st, 32 * wave, lane);
#pragma unroll
                for (int t = 0; t < NT; ++t) {
                    const bf16x8 bf = tr_fragment(Ds, LDD, 16 * st, 32 * t, lane);
                    acc[t] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(af, bf, acc[t], 0, 0, 0);
                }
            }
        }
        __syncthreads();
    }
    float* out = slab + (long long)chunk * (K + 1) * s.Cout;
    if (wlive) {
#pragma unroll
        for (int t = 0; t < NT; ++t)
#pragma unroll
            for (int r = 0; r < 16; ++r)
                out[(long long)((kb0 + wave) * 32 + mfma32_row(lane, r)) * s.Cout + n0 + 32 * t + (lane & 31)] = acc[t][r];
    }
    if (kgx == 0) {
        // bias row: thread's four columns are c4b = 4 (tid % (BN/4)) (NTHR is a multiple of BN/4); add the threads in fixed order
        *reinterpret_cast<f32x4*>(&red[tid * 4]) = colsum;
        __syncthreads();
        if (tid < BN) {
            const int grp = tid >> 2, comp = tid & 3;
            float t = 0.f;
            for (int u = grp; u < NTHR; u += BN / 4) t += red[u * 4 + comp];
            out[(long long)K * s.Cout + n0 + tid] = t;
        }
    }
}

}  // namespace rcnx
