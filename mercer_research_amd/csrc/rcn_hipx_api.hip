// rcn_hipx_api.hip -- C ABI of include/rcn_hipx.h (Track X: trainable conv net; no reference counterpart) over convnet.hpp.
#include "../../include/rcn_hipx.h"

#include <hip/hip_runtime.h>

#include <cmath>
#include <cstddef>
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <map>
#include <mutex>
#include <new>
#include <random>
#include <string>
#include <tuple>
#include <type_traits>
#include <vector>

#include "convnet.hpp"
#include "convnet_bf16.hpp"
#include "convnet_loss.hpp"
#include "convnet_epoch.hpp"
#include "convnet_metrics.hpp"
#include "convnet_halo.hpp"
#include "convnet_halo_bf16.hpp"
#include "convnet_select.hpp"
#include "convnet_update.hpp"
#include "convnet_accum.hpp"
#include "convnet_dropout.hpp"
#include "convnet_state.hpp"
#include "convnet_bn.hpp"
#include "convnet_gap.hpp"
#include "convnet_pw.hpp"
#include "convnet_dw.hpp"
#include "convnet_dw_s2.hpp"
#include "convnet_kinds.hpp"

using namespace rcnx;

namespace {

// device memory that frees itself (the device that allocated it must be current: rcn_hipx_destroy); move-only
struct Buf {
    void* p = nullptr; size_t cap = 0;
    Buf() = default;
    Buf(Buf&& o) noexcept : p(o.p), cap(o.cap) { o.p = nullptr; o.cap = 0; }
    ~Buf() { if (p) (void)hipFree(p); }
    hipError_t ensure(size_t bytes) {
        if (bytes <= cap) return hipSuccess;
        if (p) (void)hipFree(p);
        p = nullptr; cap = 0;
        const size_t want = bytes < 4096 ? 4096 : bytes;
        hipError_t e = hipMalloc(&p, want);
        if (e == hipSuccess) cap = want;
        return e;
    }
};

// what a layer IS (all that a dry-run net copies: copy_layer_table) ...
struct LayerShape {
    int kind;
    int H, W, Cin;          // input of the layer
    int oH, oW, Cout;       // output (logical Cout)
    int CoutP;              // padded to a multiple of 32
    int K;                  // contraction length (3*3*Cin or Cin*H*W for dense)
    long long w_off = 0, b_off = 0;       // padded flat layout
    long long lw_off = 0, lb_off = 0;     // logical flat layout
    bool pool_follows = false;
    // a skip (RCN_HIPX_BN_ADD_RELU: identity; RCN_HIPX_BN_ADD_RELU_DOWN: subsampled and zero-padded): the layer whose output this layer
    // adds in front of its ReLU, and -- in that source -- the layer that adds its output; -1: none
    int skip_src = -1, skip_by = -1;
    const KindRow& row() const { return kind_row(kind); }
    // its [W | b] block is taps x cin rows (+ the bias row) of CoutP columns: a 3x3 convolution 9 x Cin, the depthwise one 9 x 1, the 1x1
    // convolution and a dense layer 1 x K, batch normalisation's [gamma | beta] 1 x 1 -- what a slab, the flipped copy and the bf16 copies hold
    int taps() const { return row().ks * row().ks; }
    int cin() const { return K / taps(); }
    // the GEMM of its forward pass at batch B: over the pixels of its input map, or over the samples (a dense layer)
    ConvShape gemm(int B) const { return row().map ? ConvShape{B, H, W, Cin, CoutP} : ConvShape{B, 1, 1, K, CoutP}; }
};
// ... and what it holds on the device
struct Layer : LayerShape {
    Buf out, idx, dout;     // activation (post-ReLU / pooled), pool arg-max, gradient wrt the layer's OUTPUT
    Buf slab;               // partial [W | b] tiles of the weight-gradient kernels (reduced for all layers at once: run_reduce_jobs)
    long long wbf_off = -1, wbb_off = -1;   // bf16 mode: this layer's transposed bf16 weight copies in net->wb16 (forward / input-gradient operand)
    // batch normalisation (convnet_bn.hpp), allocated by rcn_hipx_create and never moved: [batch mean | batch invstd | running mean | running var],
    // C floats each, and the partial sums of the statistics and of the backward pass, bn_parts(max M) x 2 x C doubles
    Buf bn, bn_part;
};

// everything a captured step bakes in: its arguments are step_core's (a first or middle micro-step keys with lr = 0 and no lr_dev: it
// applies no rate, so one graph per B serves every rate and schedule)
struct StepKey {
    const float* x; const int32_t* labels; const int32_t* labels_b; const float* weight; int B; float lr; const float* lr_dev; float* loss; int micro = kWholeStep;
    auto tie() const { return std::tie(x, labels, labels_b, weight, B, lr, lr_dev, loss, micro); }
    bool operator<(const StepKey& o) const { return tie() < o.tie(); }
};
// the second label of every sample and the weight of the first (a device scalar; nullptr: 1) of a step on pair labels; none: labels_b == nullptr
struct Pair { const int32_t* labels_b = nullptr; const float* weight = nullptr; };

}  // namespace

// precision, store16, tiling and the kernel-selection options are the net's Selection (convnet_select.hpp): all that choosing a kernel reads;
// the optimiser, the loss, the average, clipping, accumulation and dropout are its Recipe: all that choosing and describing an update (and
// the dropout launches of a training forward) reads
struct rcn_hipx_net : Selection, Recipe {
    int device = 0, in_h = 0, in_w = 0, in_c = 0, max_batch = 0, classes = 0;
    hipStream_t stream = nullptr; bool own_stream = false;
    // The backward pass can run a layer's weight gradient on a second stream beside the input-gradient chain: the two only share dZ,
    // and each of these kernels leaves CUs idle while it ramps up and drains (rcn_hipx_set_overlap: 1 = every layer, 2 = dense layers).
    // OFF by default: measured no gain on the CIFAR step (fp32 0.420 / 0.418 / 0.418 ms for 0 / 1 / 2; 7 % slower while a reduction
    // launch per layer still ran on the second stream) -- the kernels are sized to fill the chip on their own.
    hipStream_t side = nullptr;
    std::vector<hipEvent_t> events; size_t ev_next = 0;
    int overlap = 0;
    bool dry = false;                       // rcn_hipx_plan: walk a step's dispatch decisions, record what WOULD be launched, touch no device
    std::string plan;
    std::vector<Layer> L;
    long long n_pad = 0, n_log = 0;
    Buf params, wt, dz, loss_part, grad_tmp, dlogits, skbuf, wb;      // wt: tap-flipped transposed weights, laid out like params (w_off)
    Buf* slab_sel = nullptr;                // where the weight-gradient launch in progress puts its partial tiles (a layer's slab)
    ReduceJobs jobs{};                      // the step's pending slab reductions
    Buf wb16; PrepJobs prep{}; long long prep_blocks = 0;      // bf16 mode: every layer's bf16 operand copies, made by ONE launch per step
    // The buffers and the state behind the Recipe.  Each is allocated once and outside any capture by the first setting that needs it
    // (reconfigure, rcn_hipx_api_update.ipp) and never moved afterwards: captured graphs hold its pointer.
    // the optimiser (convnet_sgd.hpp): `vel` (n_pad floats, laid out like params), by the first nonzero momentum
    Buf vel;
    // Adam (convnet_adam.hpp): the moments `adam_m`, `adam_v` (n_pad floats each, laid out like params) and the 32-byte AdamTick the device
    // advances, all three by the first rcn_hipx_set_adam; they survive a switch back to SGD, as the velocity survives a switch to Adam
    Buf adam_m, adam_v, adam_tick;
    // the average of the parameters (convnet_ema.hpp): `ema` (n_pad floats, laid out like params), by the first decay > 0
    Buf ema;
    // clipping by global norm (convnet_clip.hpp): the first max_norm > 0 allocates the step's gradient buffer (n_pad floats), k_grad_sumsq's partials
    // (ceil(n_pad / 4096) doubles) and the state [8-byte step counter][norm][coef].  clip_log: the caller's ring of norms
    // (rcn_hipx_set_grad_norm_log), a kernel argument.  norm_part: the scratch of rcn_hipx_grad_norm_dev, its own (it may grow; no graph
    // of the net points into it).
    Buf clip_grad, clip_part, clip_state;
    float* clip_log = nullptr; long long clip_log_cap = 0;
    Buf norm_part;
    // gradient accumulation (convnet_accum.hpp): every accum_k consecutive training micro-steps form one update.  `accum` (n_pad floats,
    // laid out like params), by the first k > 1.  accum_pos: micro-steps already accumulated in the open cycle, 0 .. k - 1 -- host state,
    // advanced when a micro-step has been enqueued.
    int accum_pos = 0;
    Buf accum;
    // dropout (convnet_dropout.hpp): the ordinal of the training forward, an int64 the device advances (k_dropout_tick), by the first p > 0
    // or the first rcn_hipx_set_dropout_state; zero at its start, never moved, and it survives what the velocity survives
    Buf drop_tick;
    // The captured steps, one cache per family (family_of): the caller's pointers plain or on pair labels (rcn_hipx_train_step_dev /
    // _pair_dev), and the epoch's steps on the net's own buffers x (rate from the host | from the device) x (mixed or not).  A family
    // that holds eight graphs and needs a ninth drops its own; drop_graphs drops them all.
    static constexpr int kFamilies = 6;
    std::map<StepKey, hipGraphExec_t> graphs[kFamilies];
    // rcn_hipx_train_epoch_dev / rcn_hipx_evaluate_dev: the batch the gather kernel fills (max_batch rows, fp32), its labels and the step's
    // loss scalar.  Allocated once, never moved: the epoch's step always sees these three pointers, so ONE captured graph per (B, lr)
    // serves every batch of every epoch, whatever set, permutation and loss slots the caller passes.
    Buf xb, yb, eloss;
    // a per-step schedule (rcn_hipx_train_epoch_ex_dev with lr_dev): the rate of the step lives in this 4-byte scalar, allocated once and
    // never moved, the update launch reads it (the _dlr forms of k_reduce_update), and ONE graph per B serves every schedule
    Buf elr;
    // mixed samples (rcn_hipx_train_epoch_mix_dev with records): the partners' labels beside yb and the step's target weight, allocated
    // once and never moved; the mixed step's loss launch reads (yb, yb2, emixw), so ONE more graph per (B, lr) / per B serves every record
    Buf yb2, emixw;
    Buf eval_part;                          // k_eval: [loss partials][correct partials][counter: zero between launches][top-k partials: 8 rows]; sized by max_batch, never moved
    long long n_instantiated = 0;           // hipGraphs instantiated since the net was created (rcn_hipx_graphs_instantiated)
    int last_rows = 0;                      // the batch of the last forward pass (rcn_hipx_last_logits_dev); 0: none yet
    bool walk_open = false;                 // between rcn_hipx_gradients_begin_dev and its last bucket: the activations belong to that walk
    // the backward pass as a resumable walk (rcn_hipx_gradients_begin_dev / _bucket_dev: a data-parallel step whose all-reduce of one bucket
    // of layers overlaps the backward pass of the layers below it)
    struct BwState {
        std::vector<char> gated;            // layer's dout already holds dZ (ReLU gate applied by the producer)
        std::vector<PooledGrad> pooled;     // layer's dZ exists only at pooled resolution
        bool side_busy = false;
        int next = -1;                      // the next layer the walk handles (it runs from the last layer down to 0)
        const float* x = nullptr; int B = 0; float* grad = nullptr;
        int taken = 0;                      // buckets handed out since rcn_hipx_gradients_begin_dev
        std::vector<int> lo;                // bucket k ends with layer lo[k] (a layer with parameters; lo.back() == the first such layer)
        std::vector<long long> off, len;    // its slice of the padded flat gradient
    } bw;
    std::string err;
};

namespace {

int fail(rcn_hipx_net* n, int code, const std::string& m) { if (n) n->err = m; return code; }
// dry run (rcn_hipx_plan): note the launch that the code in front of this call has decided on and tell the caller to return
bool dry_note(rcn_hipx_net* n, const char* fmt, ...) {
    if (!n->dry) return false;
    char buf[512];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof buf, fmt, ap);
    va_end(ap);
    n->plan += buf;
    n->plan += "\n";
    return true;
}
#define XTRY(net, expr) do { hipError_t e_ = (expr); if (e_ != hipSuccess) return fail(net, e_ == hipErrorOutOfMemory ? -7 : -4, std::string(#expr) + ": " + hipGetErrorString(e_)); } while (0)
#define RTRY(expr) do { int s_ = (expr); if (s_ != 0) return s_; } while (0)

void drop_graphs(rcn_hipx_net* n);
// scratch buffers that captured graphs point into: one that grows moves, and every cached graph would replay on freed memory --
// drop them, they are re-captured on demand (sizes are settled by the eager step that precedes every capture)
hipError_t scratch_ensure(rcn_hipx_net* n, Buf& b, size_t bytes) {
    if (n->dry) return hipSuccess;
    const void* before = b.p;
    const hipError_t e = b.ensure(bytes);
    if (e == hipSuccess && before && b.p != before) drop_graphs(n);
    return e;
}

struct Dev { int prev = -1; explicit Dev(int d) { (void)hipGetDevice(&prev); if (prev != d) (void)hipSetDevice(d); else prev = -1; } ~Dev() { if (prev >= 0) (void)hipSetDevice(prev); } };

int grid1d(long long total, int block) { long long g = (total + block - 1) / block; return (int)(g < 1 ? 1 : (g > 4096 ? 4096 : g)); }

// RCN_HIPX_HALO_F32 only seeds a new net's tiling mode (rcn_hipx_create); rcn_hipx_set_tiling changes it per net
static int halo_f32_default() { const char* e = std::getenv("RCN_HIPX_HALO_F32"); const int v = e ? std::atoi(e) : 1; return v < 0 || v > 2 ? 1 : v; }

// workgroups of `kernel` (256 threads; static LDS only, or -- a k_pw instantiation -- `dyn_lds` bytes of dynamic LDS) the device holds at
// once: the grid of a kernel whose workgroups loop over work items.  Asked from the runtime once per (device, kernel, LDS size).  The
// option halo_f32_slots stands for the answer for the static-LDS kernels, not for k_pw (select_pw sizes that grid from the option itself);
// where the runtime gives none: two workgroups per CU of a static-LDS kernel, one of k_pw.
long long resident_slots(rcn_hipx_net* n, const void* kernel, size_t dyn_lds = 0) {
    if (!dyn_lds && n->opt.halo_f32_slots > 0) return n->opt.halo_f32_slots;
    static std::mutex mu;
    static std::map<std::tuple<int, const void*, size_t>, long long> cache;
    const std::lock_guard<std::mutex> lock(mu);
    const std::tuple<int, const void*, size_t> key{n->device, kernel, dyn_lds};
    auto it = cache.find(key);
    if (it != cache.end()) return it->second;
    int per_cu = 0, cus = 0;
    if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, kernel, kThreads, dyn_lds) != hipSuccess || per_cu < 1) per_cu = dyn_lds ? 1 : 2;
    if (hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, n->device) != hipSuccess || cus < 1) cus = 256;
    const long long v = (long long)per_cu * cus;
    cache.emplace(key, v);
    return v;
}
// a looping kernel over `items` work items: at most as many workgroups as the chip holds at once, each taking items blockIdx.x, + gridDim.x, ...
template <typename... P, typename... A> void launch_resident(rcn_hipx_net* n, void (*kernel)(P...), long long items, A... args) {
    const long long slots = resident_slots(n, (const void*)kernel);
    hipLaunchKernelGGL(kernel, dim3((unsigned)(items < slots ? items : slots)), dim3(kThreads), 0, n->stream, args...);
}

// layer i's out / dout are bf16 tensors (i < 0: the net's input, always fp32)
bool stage16(const rcn_hipx_net* n, int i) { return n->store16 && i >= 0 && (n->L[i].kind == RCN_HIPX_CONV3X3_RELU || n->L[i].kind == RCN_HIPX_MAXPOOL2); }

// From a run-time value to a template argument: f(std::integral_constant<int, V>{}) for the V of the list that equals v -- the LAST of the
// list when none does (the selectors only hand out listed values).  The lists at the call sites are the set of kernels the library holds.
template <int V, int... Rest, typename F> void with_const(int v, F&& f) {
    if constexpr (sizeof...(Rest) == 0) f(std::integral_constant<int, V>{});
    else if (v == V) f(std::integral_constant<int, V>{});
    else with_const<Rest...>(v, f);
}
template <typename F> void with_bool(bool v, F&& f) { if (v) f(std::true_type{}); else f(std::false_type{}); }
// a tensor's storage type: __bf16 or float
template <typename T> struct Type { using type = T; };
template <typename F> void with_storage(bool is16, F&& f) { if (is16) f(Type<__bf16>{}); else f(Type<float>{}); }
// ... and a resident set's row type: uint8_t or float
template <typename F> void with_row_type(bool u8, F&& f) { if (u8) f(Type<uint8_t>{}); else f(Type<float>{}); }
// (epilogue, pooled-resolution input) of the LDS-tiled forward kernels: a pooled-resolution input only occurs in the input-gradient pass
// (EPI 0 / 3); false: no such kernel
template <typename F> bool with_epi_pin(int kepi, bool pin, F&& f) {
    if (pin && kepi != 0 && kepi != 3) return false;
    if (pin) with_const<3, 0>(kepi, [&](auto EPI) { f(EPI, std::true_type{}); });
    else with_const<0, 1, 2, 3, 4>(kepi, [&](auto EPI) { f(EPI, std::false_type{}); });
    return true;
}
#define CV(c_) (decltype(c_)::value)        /* the value of one of those constants, as a template argument */
#define CT(t_) typename decltype(t_)::type   /* ... and the type in a Type<> */

// operands rounded to bf16: *WB is the prepared transposed copy [Cout][Kp] of the K x Cout weights (prep_bf16_weights), or -- none prepared --
// made here into the shared scratch, in front of the launch that reads it; the activations are rounded inside the kernel
int bf16_operand(rcn_hipx_net* n, const float* Wk, int K, int Cout, const __bf16** WB) {
    if (*WB) return 0;
    const int Kp = (K + 31) / 32 * 32;
    XTRY(n, scratch_ensure(n, n->wb, (size_t)Cout * Kp * sizeof(__bf16)));
    hipLaunchKernelGGL(k_prep_weights_bf16, dim3(grid1d((long long)Cout * Kp, 256)), dim3(256), 0, n->stream, Wk, K, Cout, (__bf16*)n->wb.p, Kp);
    *WB = (const __bf16*)n->wb.p;
    return 0;
}

// Y = act(conv(X) + b): the kernel select_conv chooses (convnet_select.hpp).  Split-K launches leave raw partial tiles in `skbuf` that
// k_splitk_epilogue sums in order.
int launch_conv(rcn_hipx_net* n, const float* X, const float* Wk, const float* bias, float* Y, ConvShape s, int ks, int epi, uint8_t* pool_idx = nullptr,
                const PooledGrad* pin = nullptr, bool force_fp32 = false, const __bf16* wb_ready = nullptr, Store st = Store{}, const std::string* note = nullptr) {
    const bool pooled = pin != nullptr;
    const ConvChoice c = select_conv(*n, s, ks, epi, pooled, force_fp32, st);
    if (c.error) return fail(n, -3, c.error);
    if (dry_note(n, "%s", (note ? *note : describe(c, s, ks, epi, pooled)).c_str())) return 0;      // (note: the plan line of a caller's own selector, launch_pw)
    const long long M = (long long)s.N * s.H * s.W;
    float* out = Y;
    if (c.Z > 1) {
        XTRY(n, scratch_ensure(n, n->skbuf, (size_t)c.Z * M * s.Cout * sizeof(float)));
        out = (float*)n->skbuf.p;
    }
    const __bf16* WB = wb_ready;                    // made for all layers at the start of the step (prep_bf16_weights)
    if (c.bf16) RTRY(bf16_operand(n, Wk, ks * ks * s.Cin, s.Cout, &WB));
    const PooledGrad pg = pin ? *pin : PooledGrad{nullptr, nullptr, nullptr};
    const dim3 grid((unsigned)((M + kBM - 1) / kBM), (unsigned)(s.Cout / c.bn), (unsigned)c.Z);      // the implicit-GEMM kernels'
    const int items = (int)c.items;
    bool found = true;
    switch (c.kernel) {
    case ConvKernel::conv1_fwd_f32:
        with_const<3, 1>(s.Cin, [&](auto CIN) { with_const<16, 8>(c.tile_w, [&](auto TW) { with_const<4, 2>(epi, [&](auto EPI) { with_storage(st.y16, [&](auto T) {
            launch_resident(n, k_conv1_fwd_f32<CV(CIN), CV(TW), CV(EPI), CT(T)>, c.items, X, Wk, bias, (CT(T)*)Y, s, c.tiles_w, c.tiles_h, items, pool_idx);
        }); }); }); });
        break;
    case ConvKernel::halo_f32:
        with_const<16, 8>(c.tile_w, [&](auto TW) { with_const<64, 32>(c.bn, [&](auto BN) { found = with_epi_pin(c.kepi, pooled, [&](auto EPI, auto PIN) {
            launch_resident(n, k_conv3x3_halo_f32<CV(TW), CV(BN), CV(EPI), CV(PIN)>, c.items, X, Wk, bias, out, s, c.tiles_w, c.tiles_h, items, pool_idx, pg);
        }); }); });
        break;
    case ConvKernel::halo_bf16p:
        with_const<32, 64>(s.Cin, [&](auto CI) { with_const<64, 32>(c.bn, [&](auto BN) { found = with_epi_pin(c.kepi, pooled, [&](auto EPI, auto PIN) { with_storage(st.x16, [&](auto T) {
            launch_resident(n, k_conv3x3_halo_bf16p<CV(CI), CV(BN), CV(EPI), CV(PIN), CT(T)>, c.items, (const CT(T)*)X, WB, bias, (CT(T)*)out, s, c.tiles_w, c.tiles_h, items, pool_idx,
                            PooledGradT<CT(T)>{(const CT(T)*)pg.dP, (const CT(T)*)pg.P, pg.idx});
        }); }); }); });
        break;
    case ConvKernel::halo_bf16p_rows16:
        with_const<32, 64>(s.Cin, [&](auto CI) { found = with_epi_pin(c.kepi, pooled, [&](auto EPI, auto PIN) {
            launch_resident(n, k_conv3x3_halo_bf16p<CV(CI), 64, CV(EPI), CV(PIN), __bf16, 2>, c.items, (const __bf16*)X, WB, bias, (__bf16*)out, s, c.tiles_w, c.tiles_h, items, pool_idx,
                            PooledGradT<__bf16>{(const __bf16*)pg.dP, (const __bf16*)pg.P, pg.idx});
        }); });
        break;
    case ConvKernel::halo_bf16_1cb:
        found = with_epi_pin(c.kepi, pooled, [&](auto EPI, auto PIN) { with_storage(st.x16, [&](auto T) {
            launch_resident(n, k_conv3x3_halo_bf16_1cb<32, CV(EPI), CV(PIN), CT(T)>, c.items, (const CT(T)*)X, WB, bias, (CT(T)*)out, s, c.tiles_w, c.tiles_h, items, pool_idx,
                            PooledGradT<CT(T)>{(const CT(T)*)pg.dP, (const CT(T)*)pg.P, pg.idx});
        }); });
        break;
    case ConvKernel::halo_bf16: {
        const dim3 hgrid((unsigned)(c.tiles_w * c.tiles_h * s.N), (unsigned)(s.Cout / c.bn));
        with_const<32, 64>(s.Cin, [&](auto CI) { with_const<64, 32>(c.bn, [&](auto BN) { with_const<0, 1, 2, 3, 4>(c.kepi, [&](auto EPI) { with_bool(pooled, [&](auto PIN) {
            hipLaunchKernelGGL((k_conv3x3_halo_bf16<CV(CI), CV(BN), CV(EPI), CV(PIN)>), hgrid, dim3(kThreads), 0, n->stream, X, WB, bias, out, s, c.tiles_w, c.tiles_h, pool_idx, pg);
        }); }); }); });
        break;
    }
    case ConvKernel::fwd_bf16_map:
        // x16: reads the bf16 map; y16: writes one -- the kernel itself where it does not split K, else k_splitk_epilogue
        with_const<128, 64, 32>(c.bn, [&](auto BN) { with_const<0, 1, 2, 3>(c.kepi, [&](auto EPI) {
            if (st.x16) hipLaunchKernelGGL((k_conv_fwd_bf16<1, false, CV(BN), CV(EPI), __bf16, float>), grid, dim3(kThreads), 0, n->stream, (const __bf16*)X, WB, bias, out, s);
            else if (c.Z == 1) hipLaunchKernelGGL((k_conv_fwd_bf16<1, false, CV(BN), CV(EPI), float, __bf16>), grid, dim3(kThreads), 0, n->stream, X, WB, bias, (__bf16*)out, s);
            else hipLaunchKernelGGL((k_conv_fwd_bf16<1, false, CV(BN), CV(EPI)>), grid, dim3(kThreads), 0, n->stream, X, WB, bias, out, s);
        }); });
        break;
    case ConvKernel::fwd_bf16:
        // (no dense gather form: a dense layer's inputs are a multiple of 32 -- describe_layers -- so select_conv never asks for <1, gather>)
        with_const<3, 1>(ks, [&](auto KS) { with_bool(c.smallc, [&](auto SM) { with_const<128, 64, 32>(c.bn, [&](auto BN) { with_const<0, 1, 2, 3>(c.kepi, [&](auto EPI) {
            if constexpr (CV(KS) == 1 && CV(SM)) found = false;
            else hipLaunchKernelGGL((k_conv_fwd_bf16<CV(KS), CV(SM), CV(BN), CV(EPI)>), grid, dim3(kThreads), 0, n->stream, X, WB, bias, out, s);
        }); }); }); });
        break;
    case ConvKernel::fwd_f32:
        with_const<3, 1>(ks, [&](auto KS) { with_bool(c.smallc, [&](auto SM) { with_const<64, 32>(c.bn, [&](auto BN) { with_const<0, 1, 2, 3>(c.kepi, [&](auto EPI) {
            if constexpr (CV(KS) == 1 && CV(SM)) found = false;      // (no dense gather form, as above)
            else hipLaunchKernelGGL((k_conv_fwd<CV(KS), CV(SM), CV(BN), CV(EPI)>), grid, dim3(kThreads), 0, n->stream, X, Wk, bias, out, s);
        }); }); }); });
        break;
    }
    if (!found) return fail(n, -3, "internal: no kernel of this form (a pooled-resolution input with a forward epilogue, or a dense layer on the gather loader)");
    XTRY(n, hipGetLastError());
    if (c.Z > 1) {
        if (st.y16) hipLaunchKernelGGL(k_splitk_epilogue<__bf16>, dim3(grid1d(M * s.Cout, 256)), dim3(256), 0, n->stream, (const float*)n->skbuf.p, bias, (__bf16*)Y, M * s.Cout, s.Cout, c.Z, epi);
        else hipLaunchKernelGGL(k_splitk_epilogue<float>, dim3(grid1d(M * s.Cout, 256)), dim3(256), 0, n->stream, (const float*)n->skbuf.p, bias, Y, M * s.Cout, s.Cout, c.Z, epi);
        XTRY(n, hipGetLastError());
    }
    return 0;
}

// the partial [W | b] tiles of a layer's weight gradient into its slab (n->slab_sel), by the kernel select_wgrad chooses; *chunks_out: how many
// st.x16: X is a bf16 tensor; st.y16: dZ (and a pooled-resolution dZ) is
int launch_wgrad(rcn_hipx_net* n, const float* X, const float* dZ, ConvShape s, int ks, int* chunks_out, const PooledGrad* pdz = nullptr, Store st = Store{}, bool map1x1 = false) {
    const bool pooled = pdz != nullptr;
    const WgradChoice c = select_wgrad(*n, s, ks, pooled, st);
    if (c.error) return fail(n, -3, c.error);
    *chunks_out = c.chunks;
    if (dry_note(n, "%s", describe(c, s, ks, pooled, map1x1).c_str())) return 0;
    const int K = ks * ks * s.Cin;
    XTRY(n, scratch_ensure(n, *n->slab_sel, (size_t)c.chunks * (K + 1) * s.Cout * sizeof(float)));
    float* const slab = (float*)n->slab_sel->p;
    const PooledGrad pg = pdz ? *pdz : PooledGrad{nullptr, nullptr, nullptr};
    switch (c.kernel) {
    case WgradKernel::conv1_wgrad_f32: {
        const dim3 grid((unsigned)(s.Cout / 32), (unsigned)c.chunks);
        with_const<3, 1>(s.Cin, [&](auto CIN) { with_const<16, 8>(c.tile_w, [&](auto TW) { with_bool(pooled, [&](auto PDZ) { with_storage(st.y16, [&](auto T) {
            hipLaunchKernelGGL((k_conv1_wgrad_f32<CV(CIN), CV(TW), CV(PDZ), CT(T)>), grid, dim3(kThreads), 0, n->stream, X, (const CT(T)*)dZ, slab, s, c.tiles_w, c.tiles_h, c.bpc,
                               PooledGradT<CT(T)>{(const CT(T)*)pg.dP, (const CT(T)*)pg.P, pg.idx});
        }); }); }); });
        break;
    }
    case WgradKernel::halo_f32: {
        const dim3 grid((unsigned)(s.Cin / 32), (unsigned)(s.Cout / 32), (unsigned)c.chunks);
        with_const<16, 8>(c.tile_w, [&](auto TW) { with_bool(pooled, [&](auto PDZ) {
            hipLaunchKernelGGL((k_wgrad3x3_halo_f32<CV(TW), CV(PDZ)>), grid, dim3(kThreads), 0, n->stream, X, dZ, slab, s, c.tiles_w, c.tiles_h, c.bpc, pg);
        }); });
        break;
    }
    case WgradKernel::halo_bf16: {
        const dim3 grid((unsigned)(s.Cin / c.cb), (unsigned)(s.Cout / c.bn), (unsigned)c.chunks);
        with_const<32, 64>(c.cb, [&](auto CB) { with_const<64, 32>(c.bn, [&](auto BN) { with_bool(pooled, [&](auto PDZ) { with_storage(st.x16, [&](auto T) {
            hipLaunchKernelGGL((k_wgrad3x3_halo_bf16<CV(CB), CV(BN), CV(PDZ), CT(T)>), grid, dim3(kWgHaloThreads), 0, n->stream, (const CT(T)*)X, (const CT(T)*)dZ, slab, s, c.tiles_w, c.tiles_h,
                               c.bpc, c.chunks, PooledGradT<CT(T)>{(const CT(T)*)pg.dP, (const CT(T)*)pg.P, pg.idx});
        }); }); }); });
        break;
    }
    case WgradKernel::wgrad_bf16: {
        const WgradGrid gd{K / 32 / c.nk, s.Cout / c.bn, c.chunks, n->opt.xcd_remap};
        const dim3 grid(gd.launch_blocks());
        with_const<3, 1>(ks, [&](auto KS) { with_const<64, 32>(c.bn, [&](auto BN) { with_const<4, 3, 2, 1>(c.nk, [&](auto NK) {
            if (st.x16) hipLaunchKernelGGL((k_conv_wgrad_bf16<CV(KS), CV(BN), CV(NK), __bf16>), grid, dim3(64 * CV(NK)), 0, n->stream, (const __bf16*)X, dZ, slab, s, c.ppc, gd);
            else hipLaunchKernelGGL((k_conv_wgrad_bf16<CV(KS), CV(BN), CV(NK)>), grid, dim3(64 * CV(NK)), 0, n->stream, X, dZ, slab, s, c.ppc, gd);
        }); }); });
        break;
    }
    case WgradKernel::wgrad_f32: {
        const WgradGrid gd{c.smallc ? 1 : K / 32, s.Cout / c.bn, c.chunks, n->opt.xcd_remap};
        const dim3 grid(gd.launch_blocks());
        with_const<3, 1>(ks, [&](auto KS) { with_bool(c.smallc, [&](auto SM) { with_const<64, 32>(c.bn, [&](auto BN) {
            hipLaunchKernelGGL((k_conv_wgrad<CV(KS), CV(SM), CV(BN)>), grid, dim3(kThreads), 0, n->stream, X, dZ, slab, s, c.ppc, gd);
        }); }); });
        break;
    }
    }
    XTRY(n, hipGetLastError());
    return 0;
}

// ---- RCN_HIPX_CONV3X3_S2 (convnet_select.hpp: implicit GEMM only)
// forward: Y = conv(X) + b over the (H/2) x (W/2) output map
int launch_conv_s2(rcn_hipx_net* n, const float* X, const float* Wk, const float* bias, float* Y, ConvShapeS2 s, int epi, const __bf16* WB) {
    const ConvS2Choice c = select_conv_s2(*n, s, epi);
    if (c.error) return fail(n, -3, c.error);
    if (dry_note(n, "%s", describe(c, s, epi).c_str())) return 0;
    const long long M = gemm_rows(s);
    float* out = Y;
    if (c.Z > 1) {
        XTRY(n, scratch_ensure(n, n->skbuf, (size_t)c.Z * M * s.Cout * sizeof(float)));
        out = (float*)n->skbuf.p;
    }
    if (c.bf16) RTRY(bf16_operand(n, Wk, 9 * s.Cin, s.Cout, &WB));
    const dim3 grid((unsigned)c.tiles, (unsigned)(s.Cout / c.bn), (unsigned)c.Z);
    if (c.bf16)
        with_const<128, 64, 32>(c.bn, [&](auto BN) { with_const<0, 1>(c.kepi, [&](auto EPI) {
            hipLaunchKernelGGL((k_conv_fwd_bf16<3, false, CV(BN), CV(EPI), float, float, ConvShapeS2>), grid, dim3(kThreads), 0, n->stream, X, WB, bias, out, s);
        }); });
    else
        with_const<64, 32>(c.bn, [&](auto BN) { with_const<0, 1>(c.kepi, [&](auto EPI) {
            hipLaunchKernelGGL((k_conv_fwd<3, false, CV(BN), CV(EPI), ConvShapeS2>), grid, dim3(kThreads), 0, n->stream, X, Wk, bias, out, s);
        }); });
    XTRY(n, hipGetLastError());
    if (c.Z > 1) {
        hipLaunchKernelGGL(k_splitk_epilogue<float>, dim3(grid1d(M * s.Cout, 256)), dim3(256), 0, n->stream, (const float*)n->skbuf.p, bias, Y, M * s.Cout, s.Cout, c.Z, epi);
        XTRY(n, hipGetLastError());
    }
    return 0;
}
// input gradient: dX (the whole H x W map, every element once) from dZ and the tap-flipped transposed weights, one launch over the parity classes
int launch_dgrad_s2(rcn_hipx_net* n, const float* dZ, const float* Wt, const float* gate, float* dX, ConvShapeS2T s, int epi, const __bf16* WB) {
    const ConvS2Choice c = select_dgrad_s2(*n, s, epi);
    if (c.error) return fail(n, -3, c.error);
    if (dry_note(n, "%s", describe(c, s, epi).c_str())) return 0;
    if (c.bf16) RTRY(bf16_operand(n, Wt, 9 * s.Cin, s.Cout, &WB));
    const dim3 grid((unsigned)(4 * c.tiles), (unsigned)(s.Cout / c.bn));
    if (c.bf16)
        with_const<64, 32>(c.bn, [&](auto BN) { with_const<3, 0>(c.kepi, [&](auto EPI) {
            hipLaunchKernelGGL((k_conv_fwd_bf16<3, false, CV(BN), CV(EPI), float, float, ConvShapeS2T>), grid, dim3(kThreads), 0, n->stream, dZ, WB, gate, dX, s);
        }); });
    else
        with_const<64, 32>(c.bn, [&](auto BN) { with_const<3, 0>(c.kepi, [&](auto EPI) {
            hipLaunchKernelGGL((k_conv_fwd<3, false, CV(BN), CV(EPI), ConvShapeS2T>), grid, dim3(kThreads), 0, n->stream, dZ, Wt, gate, dX, s);
        }); });
    XTRY(n, hipGetLastError());
    return 0;
}
// weight gradient into the layer's slab (n->slab_sel), as launch_wgrad
int launch_wgrad_s2(rcn_hipx_net* n, const float* X, const float* dZ, ConvShapeS2 s, int* chunks_out) {
    const WgradChoice c = select_wgrad_s2(*n, s);
    if (c.error) return fail(n, -3, c.error);
    *chunks_out = c.chunks;
    if (dry_note(n, "%s", describe(c, s).c_str())) return 0;
    const int K = 9 * s.Cin;
    XTRY(n, scratch_ensure(n, *n->slab_sel, (size_t)c.chunks * (K + 1) * s.Cout * sizeof(float)));
    float* const slab = (float*)n->slab_sel->p;
    switch (c.kernel) {
    case WgradKernel::wgrad_bf16: {
        const WgradGrid gd{K / 32 / 3, s.Cout / c.bn, c.chunks, n->opt.xcd_remap};
        with_const<64, 32>(c.bn, [&](auto BN) {
            hipLaunchKernelGGL((k_conv_wgrad_bf16<3, CV(BN), 3, float, ConvShapeS2>), dim3(gd.launch_blocks()), dim3(64 * 3), 0, n->stream, X, dZ, slab, s, c.ppc, gd);
        });
        break;
    }
    default: {
        const WgradGrid gd{K / 32, s.Cout / c.bn, c.chunks, n->opt.xcd_remap};
        with_const<64, 32>(c.bn, [&](auto BN) {
            hipLaunchKernelGGL((k_conv_wgrad<3, false, CV(BN), ConvShapeS2>), dim3(gd.launch_blocks()), dim3(kThreads), 0, n->stream, X, dZ, slab, s, c.ppc, gd);
        });
        break;
    }
    }
    XTRY(n, hipGetLastError());
    return 0;
}

// hipFuncAttributeMaxDynamicSharedMemorySize of a k_pw instantiation, set once per (device, kernel): a function's attribute belongs to
// the device's copy of it, so a net on a second device asks again (the net's device is current: every entry point holds a Dev)
hipError_t pw_allow_lds(rcn_hipx_net* n, const void* kernel) {
    static std::mutex mu;
    static std::map<std::pair<int, const void*>, hipError_t> done;
    const std::lock_guard<std::mutex> lock(mu);
    const std::pair<int, const void*> key{n->device, kernel};
    auto it = done.find(key);
    if (it != done.end()) return it->second;
    const hipError_t e = hipFuncSetAttribute(kernel, hipFuncAttributeMaxDynamicSharedMemorySize, 96 * 1024);
    done.emplace(key, e);
    return e;
}

// ---- RCN_HIPX_CONV1X1 (convnet_select.hpp: select_pw): Y = X W + b (epi 1) or the input gradient dZ Wt (epi 0 raw, 3 gated by `bias`, a tensor
// shaped like Y) over the H x W map; every element of Y is written exactly once.  s.Cin: the contraction, s.Cout: the launch's columns.
int launch_pw(rcn_hipx_net* n, const float* X, const float* Wk, const float* bias, float* Y, ConvShape s, int epi, const __bf16* WB) {
    const PwChoice c = select_pw(*n, s, epi);
    if (c.error) return fail(n, -3, c.error);
    const std::string line = describe(c, s, epi);
    if (!c.stream) return launch_conv(n, X, Wk, bias, Y, s, 1, epi, nullptr, nullptr, false, WB, Store{}, &line);
    if (dry_note(n, "%s", line.c_str())) return 0;
    if (c.bf16) RTRY(bf16_operand(n, Wk, s.Cin, s.Cout, &WB));
    const long long M = (long long)s.N * s.H * s.W;
    const size_t lds = pw_lds_bytes(c.bf16, s.Cin, c.nb);
    const void* const W = c.bf16 ? (const void*)WB : (const void*)Wk;
    int status = 0;
    with_bool(c.bf16, [&](auto B16) { with_const<1, 2, 3, 4, 5, 6, 7, 8>(c.nb / 32, [&](auto NT) { with_const<1, 3, 0>(epi, [&](auto EPI) {
        auto* const kernel = k_pw<CV(B16), CV(NT), CV(EPI)>;
        // more than 64 KB of dynamic LDS has to be asked for (at most 80 KB here), once per (device, kernel)
        const hipError_t attr = pw_allow_lds(n, (const void*)kernel);
        if (attr != hipSuccess) { status = fail(n, -4, std::string("hipFuncSetAttribute(k_pw): ") + hipGetErrorString(attr)); return; }
        // the resident grid: as many workgroups as the chip holds of this kernel with this much LDS, dealt over the column slices
        long long gx = c.grid;
        if (!gx) {
            gx = resident_slots(n, (const void*)kernel, lds) / c.passes;
            if (gx < 1) gx = 1;
            if (gx > c.items) gx = c.items;
        }
        hipLaunchKernelGGL(kernel, dim3((unsigned)gx, (unsigned)c.passes), dim3(kThreads), lds, n->stream, X, W, bias, Y, M, s.Cin, s.Cout);
    }); }); });
    if (status) return status;
    XTRY(n, hipGetLastError());
    return 0;
}

// ---- RCN_HIPX_DWCONV3X3 (convnet_select.hpp: select_dw): Y = dwconv(X, W) + b (epi 1), or the input gradient -- the same stencil over dZ on the
// tap-reversed copy (epi 0 raw, 3 gated by `bias`, a tensor shaped like Y); fp32 in either precision mode.  The tiles partition the map and
// a lane stores each of its pieces once: every element of Y is written exactly once, by one thread.
int launch_dw(rcn_hipx_net* n, const float* X, const float* Wk, const float* bias, float* Y, ConvShape s, int epi) {
    const DwChoice c = select_dw(*n, s, epi);
    if (c.error) return fail(n, -3, c.error);
    if (dry_note(n, "%s", describe(c, s, epi).c_str())) return 0;
    with_const<1, 3, 0>(epi, [&](auto EPI) {
        auto* const kernel = k_dw<CV(EPI)>;
        // the resident grid: as many workgroups as the chip holds of this kernel (the option halo_f32_slots: that many), looping over the tiles
        long long gx = c.grid;
        if (!gx) { gx = resident_slots(n, (const void*)kernel); if (gx > c.items) gx = c.items; }
        hipLaunchKernelGGL(kernel, dim3((unsigned)gx), dim3(kThreads), 0, n->stream, X, Wk, bias, Y, s.H, s.W, s.Cin, c.th, c.items);
    });
    XTRY(n, hipGetLastError());
    return 0;
}
// ... and the partial [10][C] tiles of its weight gradient into the layer's slab (n->slab_sel), one per chunk of pixels; *chunks_out: how many
int launch_dw_wgrad(rcn_hipx_net* n, const float* X, const float* dZ, ConvShape s, int* chunks_out) {
    const DwWgradChoice c = select_dw_wgrad(*n, s);
    if (c.error) return fail(n, -3, c.error);
    *chunks_out = c.chunks;
    if (dry_note(n, "%s", describe(c, s).c_str())) return 0;
    XTRY(n, scratch_ensure(n, *n->slab_sel, (size_t)c.chunks * 10 * s.Cout * sizeof(float)));
    hipLaunchKernelGGL(k_dw_wgrad, dim3((unsigned)c.chunks, (unsigned)c.groups), dim3(kThreads), 0, n->stream, X, dZ, (float*)n->slab_sel->p, (long long)s.N * s.H * s.W, s.H, s.W, s.Cin,
                       c.ppc);
    XTRY(n, hipGetLastError());
    return 0;
}

// ---- RCN_HIPX_DWCONV3X3_S2 (convnet_dw_s2.hpp; convnet_select.hpp: select_dw_s2*), s: the layer's INPUT map, fp32 in either precision mode.
// forward: Y = dwconv(X, W, stride 2) + b over the (H/2) x (W/2) output map
int launch_dw_s2(rcn_hipx_net* n, const float* X, const float* Wk, const float* bias, float* Y, ConvShape s) {
    const DwChoice c = select_dw_s2(*n, s, 1);
    if (c.error) return fail(n, -3, c.error);
    if (dry_note(n, "%s", describe_dw_s2(c, s, 1).c_str())) return 0;
    long long gx = c.grid;
    if (!gx) { gx = resident_slots(n, (const void*)k_dw_s2_fwd); if (gx > c.items) gx = c.items; }
    hipLaunchKernelGGL(k_dw_s2_fwd, dim3((unsigned)gx), dim3(kThreads), 0, n->stream, X, Wk, bias, Y, s.H, s.W, s.Cin, c.th, c.items);
    XTRY(n, hipGetLastError());
    return 0;
}
// input gradient: dX (the whole H x W map) from dZ and W AS STORED (the kernel picks the taps of each parity class itself), epi 0 raw or 3
// gated by `gate`, a tensor shaped like dX.  The 2 x 2 blocks partition the map and a lane stores each of its four pieces once: ONE launch
// writes every element of dX exactly once, by one thread.
int launch_dw_s2_dgrad(rcn_hipx_net* n, const float* dZ, const float* Wk, const float* gate, float* dX, ConvShape s, int epi) {
    const DwChoice c = select_dw_s2_dgrad(*n, s, epi);
    if (c.error) return fail(n, -3, c.error);
    if (dry_note(n, "%s", describe_dw_s2_dgrad(c, s, epi).c_str())) return 0;
    with_const<3, 0>(epi, [&](auto EPI) {
        auto* const kernel = k_dw_s2_dgrad<CV(EPI)>;
        long long gx = c.grid;
        if (!gx) { gx = resident_slots(n, (const void*)kernel); if (gx > c.items) gx = c.items; }
        hipLaunchKernelGGL(kernel, dim3((unsigned)gx), dim3(kThreads), 0, n->stream, dZ, Wk, gate, dX, s.H, s.W, s.Cin, c.th, c.items);
    });
    XTRY(n, hipGetLastError());
    return 0;
}
// the partial [10][C] tiles of its weight gradient into the layer's slab (n->slab_sel), one per chunk of OUTPUT pixels; *chunks_out: how many
int launch_dw_s2_wgrad(rcn_hipx_net* n, const float* X, const float* dZ, ConvShape s, int* chunks_out) {
    const DwWgradChoice c = select_dw_s2_wgrad(*n, s);
    if (c.error) return fail(n, -3, c.error);
    *chunks_out = c.chunks;
    if (dry_note(n, "%s", describe_dw_s2_wgrad(c, s).c_str())) return 0;
    XTRY(n, scratch_ensure(n, *n->slab_sel, (size_t)c.chunks * 10 * s.Cout * sizeof(float)));
    hipLaunchKernelGGL(k_dw_s2_wgrad, dim3((unsigned)c.chunks, (unsigned)c.groups), dim3(kThreads), 0, n->stream, X, dZ, (float*)n->slab_sel->p, (long long)s.N * (s.H / 2) * (s.W / 2), s.H,
                       s.W, s.Cin, c.ppc);
    XTRY(n, hipGetLastError());
    return 0;
}

float* P(rcn_hipx_net* n, long long off) { return (float*)n->params.p + off; }

int ensure_batch(rcn_hipx_net* n, int B) {
    if (B < 1 || B > n->max_batch) return fail(n, -1, "batch size out of range for this net (max_batch)");
    return 0;
}

// `to` waits for everything enqueued on `from` so far (an event from the net's pool; inside a capture this is a graph dependency)
int stream_after(rcn_hipx_net* n, hipStream_t from, hipStream_t to) {
    if (n->ev_next == n->events.size()) {
        hipEvent_t e = nullptr;
        XTRY(n, hipEventCreateWithFlags(&e, hipEventDisableTiming));
        n->events.push_back(e);
    }
    hipEvent_t ev = n->events[n->ev_next++];
    XTRY(n, hipEventRecord(ev, from));
    XTRY(n, hipStreamWaitEvent(to, ev, 0));
    return 0;
}

bool head_fusable(const rcn_hipx_net* n);

// bf16 mode: a layer's prepared bf16 operand copy (nullptr: none -- launch_conv then makes its own)
const __bf16* wb_of(const rcn_hipx_net* n, long long off) {
    return (n->precision == RCN_HIPX_BF16 && n->wb16.p && off >= 0) ? (const __bf16*)n->wb16.p + off : (const __bf16*)nullptr;
}

// ---- The three passes of a matrix layer, by kind: the only places that switch on the convolution kind.  Each builds the shape its kind's
// launcher takes from the layer and the batch (H x W: the layer's INPUT map; a strided layer's output is l.oH x l.oW).
// The forward pass of a bias-only layer in front of batch normalisation: Y = conv(X) + b (epilogue 1), no conv+pool fusion
int layer_forward(rcn_hipx_net* n, const Layer& l, int B, const float* X, float* Y) {
    const float *const W = P(n, l.w_off), *const b = P(n, l.b_off);
    const __bf16* const WB = wb_of(n, l.wbf_off);
    switch (l.kind) {
    case RCN_HIPX_CONV3X3_S2: return launch_conv_s2(n, X, W, b, Y, ConvShapeS2{B, l.H, l.W, l.Cin, l.CoutP}, 1, WB);
    case RCN_HIPX_CONV1X1: return launch_pw(n, X, W, b, Y, l.gemm(B), 1, WB);
    case RCN_HIPX_DWCONV3X3: return launch_dw(n, X, W, b, Y, l.gemm(B), 1);
    case RCN_HIPX_DWCONV3X3_S2: return launch_dw_s2(n, X, W, b, Y, l.gemm(B));
    default: return launch_conv(n, X, W, b, Y, l.gemm(B), l.row().ks, 1, nullptr, nullptr, false, WB);
    }
}
// Its input gradient: dX = conv(dZ, flip(W)^T) on the tap-flipped transposed weights, which every kernel that writes a weight keeps current
// (FlipSpec, refresh_flipped).  gate_by (nullable): the ReLU layer below, whose output gates dX in the epilogue (3; else 0, raw).  pdz
// (nullable): dZ exists only at pooled resolution; st: dZ / dX are bf16 tensors.  Whatever the kind, ONE launch writes ALL of dX, every element
// once and with no accumulation: a strided layer over the four parity classes of the input pixels, k_dw's tiles partitioning the map,
// k_dw_s2_dgrad's 2 x 2 blocks partitioning it.
int layer_dgrad(rcn_hipx_net* n, const Layer& l, int B, const float* dZ, const Layer* gate_by, float* dX, const PooledGrad* pdz, Store st) {
    const float *const wt = (const float*)n->wt.p + l.w_off, *const gate = gate_by ? (const float*)gate_by->out.p : nullptr;
    const int epi = gate_by ? 3 : 0;
    const __bf16* const WB = wb_of(n, l.wbb_off);
    const ConvShape s = l.gemm(B), t{s.N, s.H, s.W, s.Cout, s.Cin};      // t: the transposed GEMM, dZ's channels contracted
    switch (l.kind) {
    case RCN_HIPX_CONV3X3_S2: return launch_dgrad_s2(n, dZ, wt, gate, dX, ConvShapeS2T{t.N, t.H, t.W, t.Cin, t.Cout}, epi, WB);
    case RCN_HIPX_CONV1X1: return launch_pw(n, dZ, wt, gate, dX, t, epi, WB);
    case RCN_HIPX_DWCONV3X3: return launch_dw(n, dZ, wt, gate, dX, s, epi);      // (the same stencil over dZ: C -> C)
    case RCN_HIPX_DWCONV3X3_S2: return launch_dw_s2_dgrad(n, dZ, P(n, l.w_off), gate, dX, s, epi);      // (W as stored: k_dw_s2_dgrad picks each parity class's taps)
    default: return launch_conv(n, dZ, wt, gate, dX, t, l.row().ks, epi, nullptr, pdz, false, WB, st);
    }
}
// Its weight gradient from its input X and dZ: the partial [W | b] tiles into n->slab_sel, *chunks of them (pdz, st: as above, X / dZ)
int layer_wgrad(rcn_hipx_net* n, const Layer& l, int B, const float* X, const float* dZ, int* chunks, const PooledGrad* pdz, Store st) {
    switch (l.kind) {
    case RCN_HIPX_CONV3X3_S2: return launch_wgrad_s2(n, X, dZ, ConvShapeS2{B, l.H, l.W, l.Cin, l.CoutP}, chunks);
    case RCN_HIPX_DWCONV3X3: return launch_dw_wgrad(n, X, dZ, l.gemm(B), chunks);
    case RCN_HIPX_DWCONV3X3_S2: return launch_dw_s2_wgrad(n, X, dZ, l.gemm(B), chunks);
    default: return launch_wgrad(n, X, dZ, l.gemm(B), l.row().ks, chunks, pdz, st, l.kind == RCN_HIPX_CONV1X1);      // (1x1: the KS = 1 kernels with rows walking the map)
    }
}

// bf16 mode, once per step / forward call: the transposed bf16 copies of every layer's weights -- [Cout][Kp] for the forward pass from W,
// [Cin][Kp'] for the input gradient from the flipped copy (which the update kernel keeps current) -- in ONE launch.  The first layer
// (fp32 kernels in either mode) has none.
// a layer's two copies: [CoutP][Kpf] of the Kf rows of W for the forward pass, [cin][Kpb] of the Kb rows of the flipped copy for the input gradient
struct CopyShapes { long long cin, Kf, Kpf, Kb, Kpb; };
CopyShapes copy_shapes(const Layer& l) {
    const long long Kf = l.K, Kb = (long long)l.taps() * l.CoutP;
    return {l.cin(), Kf, (Kf + 31) / 32 * 32, Kb, (Kb + 31) / 32 * 32};
}
int prep_bf16_weights(rcn_hipx_net* n) {
    if (n->precision != RCN_HIPX_BF16) return 0;
    // the path is decided before the plan is noted: two jobs per matrix layer behind layer 0, and one launch takes kMaxPrepJobs of them
    int matrices = 0;
    for (size_t i = 1; i < n->L.size(); ++i) matrices += n->L[i].row().gemm;
    if (2 * matrices > kMaxPrepJobs) {
        // more than one launch takes: no prepared copies -- every bf16 launch makes its own in front of itself (launch_conv), all into the
        // one scratch n->wb, which the stream's order keeps whole until that launch has read it
        (void)dry_note(n, "  bf16 operand copies: none prepared (%d matrix layers behind layer 0, one launch takes %d): k_prep_weights_bf16 in front of every bf16 launch, into one shared scratch",
                       matrices, kMaxPrepJobs / 2);
        return 0;
    }
    if (dry_note(n, "  bf16 operand copies of every layer's weights, both orientations: k_prep_all_bf16 (one launch)")) return 0;
    if (!n->wb16.p) {
        long long off = 0, blocks = 0;
        for (size_t i = 1; i < n->L.size(); ++i) {
            Layer& l = n->L[i];
            if (!l.row().gemm) continue;
            const CopyShapes c = copy_shapes(l);
            l.wbf_off = off; off += (long long)l.CoutP * c.Kpf;
            l.wbb_off = off; off += c.cin * c.Kpb;
            off = (off + 63) / 64 * 64;
        }
        XTRY(n, n->wb16.ensure((size_t)(off > 0 ? off : 1) * sizeof(__bf16)));
        n->prep.njobs = 0;
        for (size_t i = 1; i < n->L.size(); ++i) {
            Layer& l = n->L[i];
            if (!l.row().gemm) continue;
            const CopyShapes c = copy_shapes(l);
            PrepJob& a = n->prep.j[n->prep.njobs++];
            a = PrepJob{(const float*)P(n, l.w_off), (__bf16*)n->wb16.p + l.wbf_off, (int)c.Kf, l.CoutP, (int)c.Kpf, (int)blocks};
            blocks += prep_job_blocks(l.CoutP, (int)c.Kpf);
            PrepJob& b = n->prep.j[n->prep.njobs++];
            b = PrepJob{(const float*)n->wt.p + l.w_off, (__bf16*)n->wb16.p + l.wbb_off, (int)c.Kb, (int)c.cin, (int)c.Kpb, (int)blocks};
            blocks += prep_job_blocks((int)c.cin, (int)c.Kpb);
        }
        n->prep_blocks = blocks;
    }
    if (n->prep.njobs) {
        hipLaunchKernelGGL(k_prep_all_bf16, dim3((unsigned)n->prep_blocks), dim3(256), 0, n->stream, n->prep);
        XTRY(n, hipGetLastError());
    }
    return 0;
}

// ---- dropout (convnet_dropout.hpp): site d is the d-th RCN_HIPX_DENSE_RELU layer
int dropout_sites(const rcn_hipx_net* n) { int d = 0; for (const Layer& l : n->L) d += l.kind == RCN_HIPX_DENSE_RELU; return d; }
// the site of layer i (a RCN_HIPX_DENSE_RELU layer)
int dropout_site_of(const rcn_hipx_net* n, size_t i) { int d = 0; for (size_t k = 0; k < i; ++k) d += n->L[k].kind == RCN_HIPX_DENSE_RELU; return d; }
unsigned dropout_blocks(long long n4) { return (unsigned)((n4 + kDropThreads - 1) / kDropThreads); }
// t += 1 on the device: the first launch of a training forward
int launch_dropout_tick(rcn_hipx_net* n) {
    if (dry_note(n, "  tick: k_dropout_tick, 1 thread (the ordinal of the training forward, on the device)")) return 0;
    hipLaunchKernelGGL(k_dropout_tick, dim3(1), dim3(1), 0, n->stream, (long long*)n->drop_tick.p);
    XTRY(n, hipGetLastError());
    return 0;
}
// a' = keep ? fl(a * s) : +0 in place over a[B][U], the draws of site d at the ordinal *t_dev (t_dev == nullptr: at t_imm)
int launch_dropout_fwd(rcn_hipx_net* n, int d, float* a, int B, int U, const long long* t_dev, long long t_imm) {
    const long long n4 = (long long)B * U / 4;
    if (dry_note(n, "  dropout site %d (%d units, p %g): k_dropout_fwd, %u workgroups", d, U, (double)n->drop_p, dropout_blocks(n4))) return 0;
    hipLaunchKernelGGL(k_dropout_fwd, dim3(dropout_blocks(n4)), dim3(kDropThreads), 0, n->stream, a, n4, U,
                       DropSpec{n->drop_seed, (unsigned long long)d << 48, n->drop_thr, n->drop_s}, t_dev, t_imm);
    XTRY(n, hipGetLastError());
    return 0;
}
// g <- fl(g * s) in place over the gated gradient in layer i's dout (a site layer), directly behind the launch that wrote it
int launch_dropout_bwd(rcn_hipx_net* n, size_t i, int B) {
    Layer& l = n->L[i];
    const long long n4 = (long long)B * l.CoutP / 4;
    if (dry_note(n, "  dropout-bwd site %d: k_dropout_bwd, %u workgroups", dropout_site_of(n, i), dropout_blocks(n4))) return 0;
    hipLaunchKernelGGL(k_dropout_bwd, dim3(dropout_blocks(n4)), dim3(kDropThreads), 0, n->stream, (float*)l.dout.p, n4, n->drop_s);
    XTRY(n, hipGetLastError());
    return 0;
}

// ---- batch normalisation (convnet_bn.hpp): a RCN_HIPX_BN_RELU layer normalises the map of the RCN_HIPX_CONV3X3 layer in front of it
inline const char* const kBnStoreGap = "bf16 storage (RCN_HIPX_BF16_STORED) does not cover batch normalisation: its maps are fp32 (RCN_HIPX_BF16 rounds the convolutions' operands and works)";
int bn_layers(const rcn_hipx_net* n) { int k = 0; for (const Layer& l : n->L) k += l.row().bn; return k; }
// a training forward needs two rows per channel at least (the unbiased variance): asked before anything is enqueued
int bn_rows_ok(rcn_hipx_net* n, int B) {
    for (const Layer& l : n->L)
        if (l.row().bn && (long long)B * l.oH * l.oW < 2) return fail(n, -2, "batch normalisation needs at least two rows (B * H * W >= 2) in a training forward");
    return 0;
}
float* bn_mean(const Layer& l) { return (float*)l.bn.p; }
float* bn_invstd(const Layer& l) { return (float*)l.bn.p + l.CoutP; }
float* bn_run_mean(const Layer& l) { return (float*)l.bn.p + 2 * l.CoutP; }
float* bn_run_var(const Layer& l) { return (float*)l.bn.p + 3 * l.CoutP; }
// running mean 0, running variance 1 in every such layer, on the net's stream
int bn_reset_stats(rcn_hipx_net* n) {
    for (const Layer& l : n->L) {
        if (!l.row().bn) continue;
        const std::vector<float> init = [&] { std::vector<float> v((size_t)4 * l.CoutP, 0.f); for (int c = 0; c < l.CoutP; ++c) v[(size_t)3 * l.CoutP + c] = 1.f; return v; }();
        XTRY(n, hipMemcpyAsync(l.bn.p, init.data(), init.size() * sizeof(float), hipMemcpyHostToDevice, n->stream));
        XTRY(n, hipStreamSynchronize(n->stream));       // (the staging vector ends here)
    }
    return 0;
}
// layer i (RCN_HIPX_BN_RELU, RCN_HIPX_BN_ADD_RELU) of a forward pass over x[M][C]: train -- the batch's statistics (two launches; the running statistics
// advance), then the apply launch on them; else the apply launch on the running statistics
int launch_bn_forward(rcn_hipx_net* n, size_t i, const float* x, int B, bool train) {
    Layer& l = n->L[i];
    const int C = l.CoutP;
    const long long M = (long long)B * l.oH * l.oW, n4 = M * (C / 4);
    const int parts = bn_parts(M);
    const unsigned blocks = bn_stream_blocks(n4, C / 4);
    if (train && !n->dry && (size_t)parts * 2 * C * sizeof(double) > l.bn_part.cap) return fail(n, -3, "internal: more partial sums than the layer's buffer holds");
    // RCN_HIPX_BN_ADD_RELU: the skip's map (the source layer's output, of this layer's shape: describe_layers) is added in front of the ReLU
    // RCN_HIPX_BN_ADD_RELU_DOWN: the source is twice as high and wide and has Cs <= C channels; it comes in through the option-A shortcut
    // RCN_HIPX_BN, RCN_HIPX_BN_ADD: the same statistics and the same expression without the ReLU, k_bn_apply<EVAL, ADD> (identity skip only)
    const bool add = l.skip_src >= 0, down = l.kind == RCN_HIPX_BN_ADD_RELU_DOWN, linear = !l.row().relu;
    const float* const skip = add ? (const float*)n->L[l.skip_src].out.p : (const float*)nullptr;
    const int Cs = down ? n->L[l.skip_src].CoutP : C;
    const SkipDown sd{l.oH, l.oW, Cs, (C - Cs) / 2};
    // geom...: nothing for k_bn_apply_relu<EVAL, ADD> (the two modes there were: their kernels take the arguments they took), or the one
    // SkipDown that k_bn_apply_relu<EVAL, true, SkipDown> takes behind eps -- the kernel's trailing parameter pack (convnet_bn.hpp)
    auto apply = [&](auto kernel, const float* mean, const float* stat2, auto... geom) {
        hipLaunchKernelGGL(kernel, dim3(blocks), dim3(kBnThreads), 0, n->stream, x, skip, (float*)l.out.p, n4, C, mean, stat2, (const float*)P(n, l.w_off), (const float*)P(n, l.b_off), n->bn_eps, geom...);
    };
    const std::string down_words = down ? strf(", subsampled (2h, 2w), its %d channels at %d .. %d", Cs, sd.lo, sd.lo + Cs - 1) : std::string();
    if (train) {
        if (!dry_note(n, "  bn-stats %dx%dx%d: k_bn_stats, %d partials of %lld rows, then k_bn_stats_finish (one workgroup, %d threads per channel; momentum %g, eps %g)",
                      l.oH, l.oW, C, parts, bn_rows_per_part(M), bn_team(C), (double)n->bn_momentum, (double)n->bn_eps)) {
            hipLaunchKernelGGL(k_bn_stats, dim3((unsigned)parts, (unsigned)bn_group_blocks(C)), dim3(kBnThreads), 0, n->stream, x, M, C, (double*)l.bn_part.p);
            XTRY(n, hipGetLastError());
            hipLaunchKernelGGL(k_bn_stats_finish, dim3(1), dim3(kBnFinishThreads), 0, n->stream, (const double*)l.bn_part.p, parts, M, C, n->bn_momentum, n->bn_eps,
                               bn_mean(l), bn_invstd(l), bn_run_mean(l), bn_run_var(l));
            XTRY(n, hipGetLastError());
        }
        if (linear) {
            if (add ? dry_note(n, "  bn-add %dx%dx%d: k_bn_apply_add, %u workgroups (no activation; the batch's mean and invstd; skip: the output of layer %d)", l.oH, l.oW, C, blocks, l.skip_src)
                    : dry_note(n, "  bn %dx%dx%d: k_bn_apply, %u workgroups (no activation; the batch's mean and invstd)", l.oH, l.oW, C, blocks)) return 0;
            if (add) apply(k_bn_apply<false, true>, bn_mean(l), bn_invstd(l)); else apply(k_bn_apply<false, false>, bn_mean(l), bn_invstd(l));
            XTRY(n, hipGetLastError());
            return 0;
        }
        if (add ? dry_note(n, "  bn-add-relu %dx%dx%d: k_bn_apply_add_relu%s, %u workgroups (the batch's mean and invstd; skip: the output of layer %d%s)", l.oH, l.oW, C, down ? "_down" : "", blocks,
                           l.skip_src, down_words.c_str())
                : dry_note(n, "  bn-relu %dx%dx%d: k_bn_apply_relu, %u workgroups (the batch's mean and invstd)", l.oH, l.oW, C, blocks)) return 0;
        if (down) apply(k_bn_apply_relu<false, true, SkipDown>, bn_mean(l), bn_invstd(l), sd);
        else if (add) apply(k_bn_apply_relu<false, true>, bn_mean(l), bn_invstd(l));
        else apply(k_bn_apply_relu<false, false>, bn_mean(l), bn_invstd(l));
    } else {
        if (linear) {
            if (add ? dry_note(n, "  bn-add %dx%dx%d: k_bn_apply_add<eval>, %u workgroups (no activation; scale and shift from the running statistics, eps %g; skip: the output of layer %d)", l.oH, l.oW, C,
                               blocks, (double)n->bn_eps, l.skip_src)
                    : dry_note(n, "  bn %dx%dx%d: k_bn_apply<eval>, %u workgroups (no activation; scale and shift from the running statistics, eps %g)", l.oH, l.oW, C, blocks, (double)n->bn_eps)) return 0;
            if (add) apply(k_bn_apply<true, true>, bn_run_mean(l), bn_run_var(l)); else apply(k_bn_apply<true, false>, bn_run_mean(l), bn_run_var(l));
            XTRY(n, hipGetLastError());
            return 0;
        }
        if (add ? dry_note(n, "  bn-add-relu %dx%dx%d: k_bn_apply_add_relu%s<eval>, %u workgroups (scale and shift from the running statistics, eps %g; skip: the output of layer %d%s)",
                           l.oH, l.oW, C, down ? "_down" : "", blocks, (double)n->bn_eps, l.skip_src, down_words.c_str())
                : dry_note(n, "  bn-relu %dx%dx%d: k_bn_apply_relu<eval>, %u workgroups (scale and shift from the running statistics, eps %g)", l.oH, l.oW, C, blocks, (double)n->bn_eps)) return 0;
        if (down) apply(k_bn_apply_relu<true, true, SkipDown>, bn_run_mean(l), bn_run_var(l), sd);
        else if (add) apply(k_bn_apply_relu<true, true>, bn_run_mean(l), bn_run_var(l));
        else apply(k_bn_apply_relu<true, false>, bn_run_mean(l), bn_run_var(l));
    }
    XTRY(n, hipGetLastError());
    return 0;
}

// ---- global average pooling (convnet_gap.hpp): a RCN_HIPX_GLOBAL_AVGPOOL layer turns the fp32 map in front of it into the dense stage's [B][C]
inline const char* const kGapStoreGap = "bf16 storage (RCN_HIPX_BF16_STORED) does not cover global average pooling: it reads an fp32 map (RCN_HIPX_BF16 rounds the convolutions' operands and works)";
// layer i (RCN_HIPX_GLOBAL_AVGPOOL) of a forward pass over x[B][H * W][C], training and evaluation alike
int launch_gap_forward(rcn_hipx_net* n, size_t i, const float* x, int B) {
    Layer& l = n->L[i];
    const int C = l.CoutP, HW = l.H * l.W;
    const dim3 grid((unsigned)B, (unsigned)gap_col_blocks(C));
    if (dry_note(n, "  gap-fwd %dx%dx%d: k_gap_fwd, %u workgroups", l.H, l.W, C, grid.x * grid.y)) return 0;
    hipLaunchKernelGGL(k_gap_fwd, grid, dim3(kGapThreads), 0, n->stream, x, (float*)l.out.p, HW, C);
    XTRY(n, hipGetLastError());
    return 0;
}
// ... and of the backward pass: its dout[B][C], which the dense layer above wrote ungated, spread over the map into the dout of the layer
// below.  gate: that layer is a ReLU layer and finds its dZ ready (the caller sets n->bw.gated); a max-pool below gates in its own backward.
int launch_gap_backward(rcn_hipx_net* n, size_t i, int B, bool gate) {
    Layer& l = n->L[i];
    Layer& below = n->L[i - 1];
    const int C = l.CoutP, HW = l.H * l.W;
    const long long n4 = (long long)B * HW * (C / 4);
    const unsigned blocks = bn_stream_blocks(n4, C / 4);
    if (dry_note(n, "  gap-bwd %dx%dx%d: k_gap_bwd, %u workgroups (%s)", l.H, l.W, C, blocks,
                 (gate ? "gated here with layer " + std::to_string(i - 1) + "'s output (out > 0)" : "ungated: layer " + std::to_string(i - 1) + " is a pool").c_str())) return 0;
    if (gate) hipLaunchKernelGGL(k_gap_bwd<true>, dim3(blocks), dim3(kBnThreads), 0, n->stream, (const float*)l.dout.p, (const float*)below.out.p, (float*)below.dout.p, n4, HW, C);
    else hipLaunchKernelGGL(k_gap_bwd<false>, dim3(blocks), dim3(kBnThreads), 0, n->stream, (const float*)l.dout.p, (const float*)nullptr, (float*)below.dout.p, n4, HW, C);
    XTRY(n, hipGetLastError());
    return 0;
}
// who gated the dout of layer i when it is not the layer itself or a pool's backward: the layer above, in the plan's words
const char* gated_above_words(const rcn_hipx_net* n, size_t i) {
    return i + 1 < n->L.size() && n->L[i + 1].kind == RCN_HIPX_GLOBAL_AVGPOOL ? "gated by the global average pool above" : "gated by the convolution above";
}

// forward for batch B; returns pointer to logits (padded rows of CoutP)
// train: the forward of a training step (step_front) -- with dropout on, every RCN_HIPX_DENSE_RELU layer's output goes through its site's
// mask; every other forward (rcn_hipx_forward_dev, evaluation) never drops and never scales
int forward(rcn_hipx_net* n, const float* x, int B, size_t n_layers = (size_t)-1, bool train = false) {
    const bool drop = train && dropout_on(*n);
    n->last_rows = B;
    const float* cur = x;
    bool cur16 = false;                                  // `cur` is a bf16 tensor (RCN_HIPX_BF16_STORED)
    if (n_layers > n->L.size()) n_layers = n->L.size();
    // (bf16 storage and a global average pool: refused with the pool's own reason, whatever the layers in front of it would say)
    if (n->store16) for (const Layer& l : n->L) if (l.kind == RCN_HIPX_GLOBAL_AVGPOOL) return fail(n, -3, kGapStoreGap);
    for (size_t i = 0; i < n_layers; ++i) {
        Layer& l = n->L[i];
        if (l.kind == RCN_HIPX_MAXPOOL2) {
            if (n->store16) return fail(n, -3, kStoreGap);          // (a pool that no convolution kernel could fuse)
            const long long tot = (long long)B * l.oH * l.oW * (l.Cin / 4);
            if (dry_note(n, "  pool %dx%dx%d: k_pool_fwd", l.H, l.W, l.Cin)) { cur = (const float*)l.out.p; continue; }
            hipLaunchKernelGGL(k_pool_fwd, dim3(grid1d(tot, 256)), dim3(256), 0, n->stream, cur, (float*)l.out.p, (uint8_t*)l.idx.p, B, l.H, l.W, l.Cin);
            XTRY(n, hipGetLastError());
        } else if (l.kind == RCN_HIPX_CONV3X3_RELU) {
            // where the pool that follows runs in this kernel's epilogue (4), only the pooled map (and its arg-max image) is written: that layer's
            const ConvShape cs = l.gemm(B);
            const bool fused = l.pool_follows && conv_pool_fusable(*n, cs);
            Layer& to = fused ? n->L[i + 1] : l;
            RTRY(launch_conv(n, cur, P(n, l.w_off), P(n, l.b_off), (float*)to.out.p, cs, 3, fused ? 4 : 2, fused ? (uint8_t*)to.idx.p : nullptr, nullptr, false, wb_of(n, l.wbf_off), Store{cur16, n->store16}));
            cur = (const float*)to.out.p;
            cur16 = n->store16;
            i += fused;
            continue;
        } else if (l.row().linear || l.row().bn) {
            // a bias-only layer (epilogue 1, no conv+pool fusion) and the batch normalisation that follows it: on fp32 maps
            if (n->store16) return fail(n, -3, kBnStoreGap);
            if (l.row().bn) RTRY(launch_bn_forward(n, i, cur, B, train)); else RTRY(layer_forward(n, l, B, cur, (float*)l.out.p));
        } else if (l.kind == RCN_HIPX_GLOBAL_AVGPOOL) {
            RTRY(launch_gap_forward(n, i, cur, B));
        } else {
            // (the logits layer of a head that training runs as k_head_f32 is fp32 here too: what bf16 mode rounds is a matter of shape)
            RTRY(launch_conv(n, cur, P(n, l.w_off), P(n, l.b_off), (float*)l.out.p, l.gemm(B), 1, l.kind == RCN_HIPX_DENSE_RELU ? 2 : 1, nullptr, nullptr,
                             i + 1 == n->L.size() && head_fusable(n), wb_of(n, l.wbf_off), Store{cur16, false}));
            if (drop && l.kind == RCN_HIPX_DENSE_RELU) RTRY(launch_dropout_fwd(n, dropout_site_of(n, i), (float*)l.out.p, B, l.CoutP, (const long long*)n->drop_tick.p, 0));
        }
        cur = (const float*)l.out.p;
        cur16 = false;
    }
    return 0;
}

// The slab of partial [W | b] tiles of layer i (chunks x (K + 1) x Cout, as the weight-gradient kernels leave it in the layer's slab)
// is queued for the step's ONE reduction launch (run_reduce_jobs): summed in chunk order, and either applied (p <- p - lr g, the flipped
// copy of the weights kept current) or written to grad.  [W | b] is contiguous (b_off == w_off + K * CoutP): one job finishes both.  Its
// geometry is the layer's own (taps, cin): a depthwise layer's n = 10 C with FlipSpec{wt, 9, 1, C}, [d gamma | d beta] n = 2 C, no flipped copy.
int reduce_slab(rcn_hipx_net* n, size_t i, int chunks, float* grad, bool apply) {
    Layer& l = n->L[i];
    if (n->jobs.njobs >= kMaxReduceJobs) return fail(n, -3, "too many layers with parameters for one reduction launch");
    ReduceJob& jb = n->jobs.j[n->jobs.njobs];
    jb.p = P(n, l.w_off);
    jb.grad = grad ? grad + l.w_off : (float*)nullptr;
    jb.slab = (const float*)l.slab.p;
    jb.flip = FlipSpec{(apply && i > 0 && l.row().matrix) ? (float*)n->wt.p + l.w_off : (float*)nullptr, l.taps(), l.cin(), l.CoutP};
    jb.n = ((long long)l.K + 1) * l.CoutP;
    if (jb.n % 4 != 0 || l.w_off % 4 != 0) return fail(n, -3, "internal: a layer's [W | b] is not a whole number of 16-byte pieces");
    jb.chunks = chunks;
    int prev_end = 0;
    if (n->jobs.njobs) { const ReduceJob& pj = n->jobs.j[n->jobs.njobs - 1]; prev_end = pj.first_block + (int)((pj.n + reduce_job_elems(pj.chunks) - 1) / reduce_job_elems(pj.chunks)); }
    jb.first_block = prev_end;
    ++n->jobs.njobs;
    return 0;
}

// Layer i (RCN_HIPX_BN_RELU) of the backward pass: the two per-channel sums of g = its dout (gated: by the pool's backward or the convolution
// above; else gated here with out > 0) into the layer's one-chunk slab [d gamma | d beta], queued for the step's reduction launch like
// any [W | b] slab (n = 2 C, no flipped copy), then the gradient of the convolution's map into that layer's dout -- its dZ.
int launch_bn_backward(rcn_hipx_net* n, size_t i, int B, bool gated, float* grad, bool apply) {
    Layer& l = n->L[i];
    Layer& cl = n->L[i - 1];
    const int C = l.CoutP;
    const long long M = (long long)B * l.oH * l.oW, n4 = M * (C / 4);
    const int parts = bn_parts(M);
    const unsigned blocks = bn_stream_blocks(n4, C / 4);
    if (!n->dry && (size_t)parts * 2 * C * sizeof(double) > l.bn_part.cap) return fail(n, -3, "internal: more partial sums than the layer's buffer holds");
    // (RCN_HIPX_BN, RCN_HIPX_BN_ADD: the caller passes gated = true for "no gate here" -- the raw dout IS the gradient of its output)
    const char* const who = !l.row().relu ? "linear: no gate" : l.pool_follows ? "gated by the pool's backward" : gated ? gated_above_words(n, i) : "gates itself (out > 0)";
    const float* const x = (const float*)cl.out.p;
    const float* const dy = (const float*)l.dout.p;
    const float* const y = (const float*)l.out.p;
    if (!dry_note(n, "  bn-bwd-reduce %dx%dx%d: k_bn_bwd_reduce, %d partials of %lld rows, then k_bn_bwd_finish (one workgroup) into the slab [d gamma | d beta]; %s",
                  l.oH, l.oW, C, parts, bn_rows_per_part(M), who)) {
        const dim3 grid((unsigned)parts, (unsigned)bn_group_blocks(C));
        if (gated) hipLaunchKernelGGL(k_bn_bwd_reduce<false>, grid, dim3(kBnThreads), 0, n->stream, x, dy, y, M, C, (const float*)bn_mean(l), (const float*)bn_invstd(l), (double*)l.bn_part.p);
        else hipLaunchKernelGGL(k_bn_bwd_reduce<true>, grid, dim3(kBnThreads), 0, n->stream, x, dy, y, M, C, (const float*)bn_mean(l), (const float*)bn_invstd(l), (double*)l.bn_part.p);
        XTRY(n, hipGetLastError());
        hipLaunchKernelGGL(k_bn_bwd_finish, dim3(1), dim3(kBnFinishThreads), 0, n->stream, (const double*)l.bn_part.p, parts, C, (float*)l.slab.p);
        XTRY(n, hipGetLastError());
    }
    if (!dry_note(n, "  bn-bwd-dx %dx%dx%d: k_bn_bwd_dx, %u workgroups (the convolution's dZ)", l.oH, l.oW, C, blocks)) {
        if (gated) hipLaunchKernelGGL(k_bn_bwd_dx<false>, dim3(blocks), dim3(kBnThreads), 0, n->stream, x, dy, y, (float*)cl.dout.p, n4, C, (float)M, (const float*)bn_mean(l),
                                      (const float*)bn_invstd(l), (const float*)P(n, l.w_off), (const float*)l.slab.p);
        else hipLaunchKernelGGL(k_bn_bwd_dx<true>, dim3(blocks), dim3(kBnThreads), 0, n->stream, x, dy, y, (float*)cl.dout.p, n4, C, (float)M, (const float*)bn_mean(l),
                                (const float*)bn_invstd(l), (const float*)P(n, l.w_off), (const float*)l.slab.p);
        XTRY(n, hipGetLastError());
    }
    return reduce_slab(n, i, 1, grad, apply);
}

// The skip's half of the backward pass of the RCN_HIPX_BN_ADD_RELU layer fed by layer `src`: that layer's dout (the gradient of the sum,
// gated like its batch-normalisation half: by the pool's backward, by the convolution above, or here with out > 0) is ADDED to dout of
// `src`, which the input-gradient kernel of layer src + 1 has just written.  src_gated: that kernel's epilogue gated dout[src] with
// out[src], so dout[src] is the source's dZ and the skip's share passes the same gate; a pool source gates in its own backward.
int launch_skip_bwd(rcn_hipx_net* n, size_t src, int B, bool src_gated) {
    Layer& s = n->L[src];
    Layer& l = n->L[s.skip_by];
    const bool linear = !l.row().relu;                   // RCN_HIPX_BN_ADD: the sum has no ReLU behind it, its dout is the skip's share as it stands
    const bool gated = linear || l.pool_follows || n->bw.gated[s.skip_by];
    // RCN_HIPX_BN_ADD_RELU_DOWN: one thread per four floats of the SMALL map's window of the source's Cs channels -- a quarter of the source map
    const bool down = l.kind == RCN_HIPX_BN_ADD_RELU_DOWN;
    const int C = l.CoutP, Cw = down ? s.CoutP : C;
    const long long n4 = (long long)B * l.oH * l.oW * (Cw / 4);
    const unsigned blocks = bn_stream_blocks(n4, Cw / 4);
    if (dry_note(n, "  skip-bwd %dx%dx%d: k_skip_bwd_add%s, %u workgroups into layer %d's gradient (the skip's gradient %s; %s)", l.oH, l.oW, Cw, down ? "_down (at (2h, 2w) of the source)" : "", blocks, (int)src,
                 linear ? "ungated: the sum has no ReLU behind it" : l.pool_follows ? "gated by the pool's backward" : gated ? gated_above_words(n, (size_t)s.skip_by) : "gated here (out > 0)",
                 (src_gated ? "then gated by layer " + std::to_string(src) + "'s output"
                            : "ungated: layer " + std::to_string(src) + (s.row().bn ? " is a batch normalisation without a ReLU" : " is a pool")).c_str())) return 0;
    auto add = [&](auto kernel) {
        hipLaunchKernelGGL(kernel, dim3(blocks), dim3(kBnThreads), 0, n->stream, (float*)s.dout.p, (const float*)l.dout.p, (const float*)l.out.p, (const float*)s.out.p, n4);
    };
    auto add_down = [&](auto kernel) {
        hipLaunchKernelGGL(kernel, dim3(blocks), dim3(kBnThreads), 0, n->stream, (float*)s.dout.p, (const float*)l.dout.p, (const float*)l.out.p, (const float*)s.out.p, n4, C,
                           SkipDown{l.oH, l.oW, Cw, (C - Cw) / 2});
    };
    with_bool(!gated, [&](auto SELF) { with_bool(src_gated, [&](auto SRC) {
        if (down) add_down(k_skip_bwd_add_down<CV(SELF), CV(SRC)>); else add(k_skip_bwd_add<CV(SELF), CV(SRC)>);
    }); });
    XTRY(n, hipGetLastError());
    return 0;
}

// the step's ONE reduction launch over the queued jobs, or the launches that stand for it (rcn_hipx_api_update.ipp)
// lr_dev (nullable): the update reads its rate from this device scalar instead of `lr` (same arithmetic on the same float)
// micro: which micro-step of an accumulating net this is (kWholeStep: the net does not accumulate, or a gradients-only walk)
int run_reduce_jobs(rcn_hipx_net* n, float lr, bool apply, const float* lr_dev = nullptr, int micro = kWholeStep);

// backward from dlogits (already in L.back().dout); apply: update parameters with lr, else write gradients to grad (padded layout).
// backward_layers handles the layers hi .. lo (downwards) and queues their slab reductions; the state that travels from layer to layer
// lives in n->bw, so the walk can stop after a bucket of layers (rcn_hipx_gradients_bucket_dev) and go on later.
int backward_layers(rcn_hipx_net* n, const float* x, int B, float lr, float* grad, bool apply, int hi, int lo, bool allow_overlap) {
    std::vector<char>& gated = n->bw.gated;
    std::vector<PooledGrad>& pooled = n->bw.pooled;
    hipStream_t const main_s = n->stream;
    struct Restore { rcn_hipx_net* n; hipStream_t s; ~Restore() { n->stream = s; } } restore{n, main_s};   // launch_* enqueue on n->stream: it is switched below
    const bool ov = allow_overlap && n->overlap && n->side;
    bool& side_busy = n->bw.side_busy;
    for (int i = hi; i >= lo; --i) {
        Layer& l = n->L[i];
        const float* in = i == 0 ? x : (const float*)n->L[i - 1].out.p;
        float* din = i == 0 ? nullptr : n->dry ? reinterpret_cast<float*>(sizeof(float)) : (float*)n->L[i - 1].dout.p;     // (dry run: no buffers; non-null = "has an input gradient")
        if (l.kind == RCN_HIPX_MAXPOOL2) {
            // When the LDS-tiled kernels run both consumers of the convolution's dZ (its weight gradient, and its input gradient if
            // it has one), they rebuild dZ from (dP, P, arg-max) at pooled resolution while staging: no k_pool_bwd, no full-size dZ.
            const Layer& cl = n->L[i - 1];
            const ConvShape cs = cl.gemm(B);
            const bool fusable = n->opt.fuse_pool_bwd && cl.kind == RCN_HIPX_CONV3X3_RELU && wgrad_halo_runs(*n, cs, 3) && (i - 1 == 0 || conv_halo_runs(*n, ConvShape{B, cl.H, cl.W, cl.CoutP, cl.Cin}));
            if (fusable) {
                pooled[i - 1] = PooledGrad{(const float*)l.dout.p, (const float*)l.out.p, (const uint8_t*)l.idx.p};
                if (dry_note(n, "  pool-bwd %dx%dx%d: none (the convolution's gradient kernels unpool while staging)", l.H, l.W, l.Cin))
                    pooled[i - 1].dP = reinterpret_cast<const float*>(sizeof(float));      // (dry run: no buffers; any non-null marks "pooled")
                continue;
            }
            // gradient wrt the pool INPUT, with the preceding conv's (or batch normalisation's) ReLU mask folded in (pooled value > 0)
            const long long tot = (long long)B * l.oH * l.oW * (l.Cin / 4);
            if (dry_note(n, "  pool-bwd %dx%dx%d: k_pool_bwd", l.H, l.W, l.Cin)) continue;
            with_storage(n->store16, [&](auto T) {
                hipLaunchKernelGGL(k_pool_bwd<CT(T)>, dim3(grid1d(tot, 256)), dim3(256), 0, n->stream, (const CT(T)*)l.dout.p, (const CT(T)*)l.out.p, (const uint8_t*)l.idx.p, (CT(T)*)din, B, l.H, l.W, l.Cin);
            });
            XTRY(n, hipGetLastError());
            continue;
        }
        if (l.kind == RCN_HIPX_GLOBAL_AVGPOOL) {
            // the layer below is a ReLU layer (describe_layers: a ReLU convolution or batch normalisation of either kind): gated here with
            // its output, so it finds its dZ ready -- no k_relu_bwd pass, the "gated" forms of the batch normalisation and skip kernels.  A
            // max-pool below gates in its own backward (k_pool_bwd, or pooled[] in the convolution below it); its dout is complete here.
            const bool gate = n->L[i - 1].kind != RCN_HIPX_MAXPOOL2;
            RTRY(launch_gap_backward(n, (size_t)i, B, gate));
            gated[i - 1] = gate;
            continue;
        }
        if (l.row().bn) {
            // its dout is gated by the pool's backward, by the convolution or by the global average pool above (n->bw.gated); otherwise it gates itself
            // RCN_HIPX_BN, RCN_HIPX_BN_ADD (no ReLU): never gated from above (the convolution above saw relu = 0: epilogue 0) and it gates nothing itself
            RTRY(launch_bn_backward(n, (size_t)i, B, !l.row().relu || l.pool_follows || gated[i], grad, apply));
            continue;
        }
        // a layer with a [W | b] block: a convolution of any kind, whose rows are the pixels of a map, or a dense layer
        const bool conv = l.row().map;
        const long long M = (long long)B * l.oH * l.oW;
        // dZ: gradient wrt the pre-activation
        const float* dZ = (const float*)l.dout.p;
        if (l.row().relu && !l.pool_follows && !gated[i]) {
            if (stage16(n, i)) return fail(n, -3, kStoreGap);
            XTRY(n, scratch_ensure(n, n->dz, (size_t)M * l.CoutP * sizeof(float)));
            if (!dry_note(n, "  relu-bwd: k_relu_bwd")) {
                hipLaunchKernelGGL(k_relu_bwd, dim3(grid1d(M * l.CoutP, 256)), dim3(256), 0, n->stream, (const float*)l.dout.p, (const float*)l.out.p, (float*)n->dz.p, M * l.CoutP);
                XTRY(n, hipGetLastError());
            }
            dZ = (const float*)n->dz.p;
        }
        // The weight gradient of this layer goes to the side stream: it needs dZ (ready on the main stream here) and the layer's
        // input.  Not when dZ sits in the shared scratch buffer, which the main stream reuses for the next layer.
        const bool on_side = ov && dZ != (const float*)n->dz.p && (n->overlap != 2 || !conv);     // 2: only the (latency-bound) dense layers
        if (on_side) { RTRY(stream_after(n, main_s, n->side)); side_busy = true; }
        const PooledGrad* const pdz = pooled[i].dP ? &pooled[i] : nullptr;      // dZ exists only at pooled resolution (the pool above fused its backward away)
        // dgrad first (needs the weights BEFORE this step's update): dX = conv(dZ, flip(W)^T)
        if (din) {
            // the layer below is a ReLU layer feeding this one directly (no pool in between): gate the gradient with its output in
            // this kernel's epilogue, so that layer finds its dZ ready instead of running a k_relu_bwd pass over the tensor
            const Layer& below = n->L[i - 1];
            // (batch normalisation below a convolution: gated here with its output, the same out > 0 rule; below a dense layer it gates itself;
            // a global average pool below has no ReLU of its own and is NOT named here: its dout stays the plain gradient of the means)
            const bool gate = below.row().relu && (!below.row().bn || conv);
            // (whatever the layer's kind, this launch writes ALL of dout[i - 1], every element once: what the skip's add below rests on)
            RTRY(layer_dgrad(n, l, B, dZ, gate ? &below : nullptr, din, pdz, Store{stage16(n, i), stage16(n, i - 1)}));
            gated[i - 1] = gate;
            if (below.kind == RCN_HIPX_DENSE_RELU && dropout_on(*n)) RTRY(launch_dropout_bwd(n, (size_t)i - 1, B));      // before anything reads that gradient
            // The layer below feeds the skip of a RCN_HIPX_BN_ADD_RELU layer further up: its gradient has a second contribution, and HERE
            // is where it is complete -- the launch above has just OVERWRITTEN dout[i - 1], and that layer's dout was finished on the main
            // stream when the walk passed it.  Nothing else touches dout[i - 1] in between: the side stream reads out[i - 1] and dout[i]
            // for this layer's weight gradient below, never dout[i - 1], and layer i - 1's own weight gradient is ordered behind this
            // point (stream_after at its iteration); a source pool's dout is read (k_pool_bwd, or pooled[] in the convolution below it)
            // only in the iterations below this one.  The add belongs to THIS iteration and gated[] lives in n->bw, so a bucket of
            // rcn_hipx_gradients_bucket_dev may end anywhere inside a block.
            // A source that is itself RCN_HIPX_BN_ADD (inverted residual blocks back to back: layer i - 1 ends block one and feeds the
            // skip of block two's RCN_HIPX_BN_ADD at skip_by > i): the add reads dout[skip_by], which was complete when the walk passed
            // skip_by + 1 -- every layer's dout is complete before the walk reaches the layer, by this same argument one block up -- and
            // completes dout[i - 1] here, BEFORE iteration i - 1 runs that layer's own batch-normalisation backward and, further down,
            // hands dout[i - 1] on as the skip's share of block one's source.  Neither share is gated: no ReLU at either sum.
            if (below.skip_by >= 0) RTRY(launch_skip_bwd(n, (size_t)i - 1, B, gate));
        }
        int chunks = 0;
        if (on_side) n->stream = n->side;
        n->slab_sel = &l.slab;
        RTRY(layer_wgrad(n, l, B, in, dZ, &chunks, pdz, Store{stage16(n, i - 1), stage16(n, i)}));
        RTRY(reduce_slab(n, (size_t)i, chunks, grad, apply));
        n->stream = main_s;
    }
    return 0;
}

void backward_reset(rcn_hipx_net* n, int first, bool first_gated) {
    n->bw.gated.assign(n->L.size(), 0);
    if (first >= 0 && first_gated) n->bw.gated[first] = 1;
    n->bw.pooled.assign(n->L.size(), PooledGrad{nullptr, nullptr, nullptr});
    n->bw.side_busy = false;
    n->ev_next = 0;
}

int backward(rcn_hipx_net* n, const float* x, int B, float lr, float* grad, bool apply, int first, bool first_gated, const float* lr_dev = nullptr, int micro = kWholeStep) {
    backward_reset(n, first, first_gated);
    RTRY(backward_layers(n, x, B, lr, grad, apply, first, 0, true));
    if (n->bw.side_busy) RTRY(stream_after(n, n->side, n->stream));   // join: the step's next kernels (and an end of capture) find everything on the main stream
    return run_reduce_jobs(n, lr, apply, lr_dev, micro);              // every layer's slab in one launch; no weight was written before this point
}

// [partial sums of the loss, one per workgroup][counter of finished workgroups: zero between launches]
int ensure_loss_buf(rcn_hipx_net* n, unsigned** counter) {
    const void* before = n->loss_part.p;
    XTRY(n, scratch_ensure(n, n->loss_part, ((size_t)n->max_batch / 8 + 2) * sizeof(float)));
    *counter = (unsigned*)n->loss_part.p + (n->max_batch / 8 + 1);
    if (n->loss_part.p != before) XTRY(n, hipMemsetAsync(n->loss_part.p, 0, n->loss_part.cap, n->stream));
    return 0;
}

// does the step's loss take a soft target (label smoothing, pair labels)?  No: the hard kernels, launched as ever
bool soft_loss(const rcn_hipx_net* n, const Pair& pair) { return n->loss_eps > 0.f || pair.labels_b != nullptr; }
// ... the plan's words for it
std::string soft_note(const rcn_hipx_net* n, const Pair& pair) {
    char buf[64];
    std::snprintf(buf, sizeof buf, ", label smoothing %g%s", (double)n->loss_eps, pair.labels_b ? ", pair labels" : "");
    return buf;
}

int loss_and_dlogits(rcn_hipx_net* n, const int32_t* labels, int B, float* loss_dev, bool want_grad, const Pair& pair = Pair{}) {
    Layer& l = n->L.back();
    const int blocks = (B + 7) / 8;                       // eight samples per workgroup
    const bool soft = soft_loss(n, pair);
    if (dry_note(n, "  loss: k_softmax_ce%s, %d workgroups%s", soft ? "_soft" : "", blocks, soft ? soft_note(n, pair).c_str() : "")) return 0;
    unsigned* counter = nullptr;
    RTRY(ensure_loss_buf(n, &counter));
    const float* const logits = (const float*)l.out.p;
    float* const dlogits = want_grad ? (float*)l.dout.p : (float*)nullptr;
    float* const part = (float*)n->loss_part.p;
    const float inv_b = 1.0f / (float)B;
    // the hard kernel, or the soft one with its one trailing argument
    auto launch = [&](auto kernel, auto... target) {
        hipLaunchKernelGGL(kernel, dim3(blocks), dim3(256), 0, n->stream, logits, labels, B, n->classes, l.CoutP, dlogits, part, counter, inv_b, loss_dev, target...);
    };
    if (soft) launch(k_softmax_ce<true, SoftTarget>, SoftTarget{pair.labels_b, pair.weight, n->loss_eps});
    else launch(k_softmax_ce<false>);
    XTRY(n, hipGetLastError());
    return 0;
}

// Does the classifier head run as one launch (k_head_f32, fp32 arithmetic in either precision mode)?  Logits layer of at most 32 classes
// on a ReLU dense layer of at most 256 units.
bool head_fusable(const rcn_hipx_net* n) {
    const int on = n->opt.head;
    // (fp32: not in GEMM tiling mode, which keeps every layer on the implicit-GEMM kernels; bf16: by shape alone -- what the mode rounds
    // must not depend on a tiling switch)
    if (!on || (n->precision == RCN_HIPX_FP32 && n->tiling == RCN_HIPX_TILING_GEMM) || n->L.size() < 2) return false;
    const Layer& l = n->L.back();
    const Layer& b = n->L[n->L.size() - 2];
    return l.kind == RCN_HIPX_DENSE && l.CoutP == 32 && l.K % 32 == 0 && l.K <= 256 && b.kind == RCN_HIPX_DENSE_RELU && b.CoutP == l.K;
}

// logits, loss, d logits, gradient into the hidden layer below (gated by its ReLU) and the logits layer's weight-gradient partials
int launch_head(rcn_hipx_net* n, const int32_t* labels, int B, float* loss_dev, int* chunks_out, const Pair& pair = Pair{}) {
    Layer& l = n->L.back();
    Layer& b = n->L[n->L.size() - 2];
    const int F = l.K, blocks = (B + 31) / 32;
    const bool soft = soft_loss(n, pair);
    *chunks_out = blocks;
    if (dry_note(n, "  head %d -> %d classes (logits, softmax + cross-entropy, gradient into the hidden layer, weight-gradient partials): k_head_f32%s, %d workgroups%s",
                 F, n->classes, soft ? "<true, true>" : "", blocks, soft ? soft_note(n, pair).c_str() : "")) return 0;
    XTRY(n, scratch_ensure(n, (*n->slab_sel), (size_t)blocks * (F + 1) * 32 * sizeof(float)));
    unsigned* counter = nullptr;
    RTRY(ensure_loss_buf(n, &counter));
    const size_t lds = ((size_t)32 * (F + 1) + (size_t)F * 32 + (size_t)32 * (F + 32) + 4 * 1024 + 1024 + 32 * 33) * sizeof(float);
    // the hard kernel, or the soft one with its one trailing argument
    auto launch = [&](auto kernel, auto... target) {
        hipLaunchKernelGGL(kernel, dim3(blocks), dim3(kThreads), lds, n->stream, (const float*)b.out.p, (const float*)P(n, l.w_off), (const float*)n->wt.p + l.w_off,
                           (const float*)P(n, l.b_off), labels, B, F, n->classes, (float*)l.out.p, (float*)b.dout.p, (float*)(*n->slab_sel).p, (float*)n->loss_part.p, counter,
                           1.0f / (float)B, loss_dev, target...);
    };
    // more than 64 KB of dynamic LDS has to be asked for (at most 127 KB here: F <= 256), once per kernel
    if (soft) {
        static const hipError_t attr_soft = hipFuncSetAttribute((const void*)k_head_f32<true, true, SoftTarget>, hipFuncAttributeMaxDynamicSharedMemorySize, 128 * 1024);
        XTRY(n, attr_soft);
        launch(k_head_f32<true, true, SoftTarget>, SoftTarget{pair.labels_b, pair.weight, n->loss_eps});
    } else {
        static const hipError_t attr = hipFuncSetAttribute((const void*)k_head_f32<true>, hipFuncAttributeMaxDynamicSharedMemorySize, 128 * 1024);
        XTRY(n, attr);
        launch(k_head_f32<true>);
    }
    XTRY(n, hipGetLastError());
    return 0;
}

// the tap-flipped transposed copy of every layer's weights that has an input gradient, from the current parameters
int refresh_flipped(rcn_hipx_net* n) {
    for (size_t i = 1; i < n->L.size(); ++i) {
        const Layer& l = n->L[i];
        if (!l.row().matrix) continue;
        hipLaunchKernelGGL(k_flip_weights, dim3(grid1d((long long)l.K * l.CoutP, 256)), dim3(256), 0, n->stream, (const float*)P(n, l.w_off), (float*)n->wt.p + l.w_off, l.row().ks, l.cin(), l.CoutP);
    }
    XTRY(n, hipGetLastError());
    return 0;
}

// The front half of a step: bf16 operand copies, forward pass, loss and d logits -- where the classifier head is the fused one, k_head_f32
// instead, which also does that layer's share of the backward pass (its slab is queued for the reduction).  *first: the layer the backward
// walk starts at; *gated: its dout already holds dZ.
int step_front(rcn_hipx_net* n, const float* x, const int32_t* labels, int B, float* grad, bool apply, float* loss_dev, int* first, bool* gated, const Pair& pair = Pair{}) {
    RTRY(bn_rows_ok(n, B));                                // (before the dropout tick and the operand copies: a refused step enqueues nothing)
    n->jobs.njobs = 0;
    if (dropout_on(*n)) RTRY(launch_dropout_tick(n));      // this forward's masks: the ordinal it leaves
    RTRY(prep_bf16_weights(n));
    const int last = (int)n->L.size() - 1;
    *gated = head_fusable(n);
    *first = *gated ? last - 1 : last;
    if (!*gated) {
        RTRY(forward(n, x, B, (size_t)-1, true));
        return loss_and_dlogits(n, labels, B, loss_dev, true, pair);
    }
    RTRY(forward(n, x, B, (size_t)last, true));
    int chunks = 0;
    n->slab_sel = &n->L[last].slab;
    RTRY(launch_head(n, labels, B, loss_dev, &chunks, pair));
    if (dropout_on(*n)) RTRY(launch_dropout_bwd(n, (size_t)last - 1, B));      // (the head wrote the gated gradient into the site layer's dout)
    return reduce_slab(n, (size_t)last, chunks, grad, apply);
}

// forward + loss + backward of one batch: parameters updated in place (apply) or gradients written to grad (padded layout)
// (lr_dev, nullable: the update's rate comes from that device scalar instead of lr; pair: a step on pair labels; micro: the micro-step of
// an accumulating net -- the front half and the backward pass are the same, only the reduction at the end differs)
int step_core(rcn_hipx_net* n, const float* x, const int32_t* labels, int B, float lr, float* grad, bool apply, float* loss_dev, const float* lr_dev = nullptr,
              const Pair& pair = Pair{}, int micro = kWholeStep) {
    int first = 0;
    bool gated = false;
    RTRY(step_front(n, x, labels, B, grad, apply, loss_dev, &first, &gated, pair));
    return backward(n, x, B, lr, grad, apply, first, gated, lr_dev, micro);
}

void drop_all(std::map<StepKey, hipGraphExec_t>& graphs) { for (auto& kv : graphs) (void)hipGraphExecDestroy(kv.second); graphs.clear(); }
// every captured graph of the net, whatever its family
void drop_graphs(rcn_hipx_net* n) { for (auto& family : n->graphs) drop_all(family); }

// ---- gradient buckets: the data-parallel step with its all-reduce overlapped with the backward pass -------------------------------------
// The layers with parameters, walked from the last to the first (the order the backward pass finishes them), are cut into buckets of at
// least min_bytes of gradient; the padded flat layout is in layer order, so a bucket is ONE contiguous slice.  Returns the bucket count.
int bucket_layout(rcn_hipx_net* n, long long min_bytes) {
    auto& bw = n->bw;
    bw.lo.clear(); bw.off.clear(); bw.len.clear();
    long long acc = 0, end = n->n_pad;
    int first_param = -1;
    for (int i = 0; i < (int)n->L.size(); ++i)
        if (n->L[i].row().params) { first_param = i; break; }
    for (int i = (int)n->L.size() - 1; i >= 0; --i) {
        const Layer& l = n->L[i];
        if (!l.row().params) continue;
        acc = (end - l.w_off) * (long long)sizeof(float);
        if (acc >= min_bytes || i == first_param) {
            bw.lo.push_back(i); bw.off.push_back(l.w_off); bw.len.push_back(end - l.w_off);
            end = l.w_off;
        }
    }
    // (the layers left over at the bottom are less than a bucket: they join the one above them)
    if (bw.lo.size() >= 2 && bw.len.back() * (long long)sizeof(float) < min_bytes) {
        const size_t m = bw.lo.size() - 1;
        bw.lo[m - 1] = bw.lo[m]; bw.off[m - 1] = bw.off[m]; bw.len[m - 1] += bw.len[m];
        bw.lo.pop_back(); bw.off.pop_back(); bw.len.pop_back();
    }
    return (int)bw.lo.size();
}

// forward, loss (and, where the classifier head is the fused one, its share of the backward pass): everything in front of bucket 0
int grad_begin(rcn_hipx_net* n, const float* x, const int32_t* labels, int B, float* grad, float* loss_dev, long long min_bytes) {
    const int nb = bucket_layout(n, min_bytes);
    n->bw.x = x; n->bw.B = B; n->bw.grad = grad; n->bw.taken = 0;
    bool gated = false;
    RTRY(step_front(n, x, labels, B, grad, false, loss_dev, &n->bw.next, &gated));
    backward_reset(n, n->bw.next, gated);
    return nb;
}

// the backward pass through bucket k's layers and the reduction of their slabs: grad[off, off + len) is final on the net's stream
int grad_bucket(rcn_hipx_net* n, int k, long long* off, long long* len) {
    auto& bw = n->bw;
    if (k < 0 || k >= (int)bw.lo.size()) return fail(n, -1, "gradients_bucket: no such bucket (rcn_hipx_gradients_begin_dev returns their number)");
    if (k != bw.taken) return fail(n, -6, "gradients_bucket: buckets are taken in order, 0 .. n - 1, after rcn_hipx_gradients_begin_dev");
    const int lo = k + 1 == (int)bw.lo.size() ? 0 : bw.lo[k];            // (the last bucket also walks whatever lies below its first layer with parameters: nothing)
    const int hi = bw.next;                                               // (hi < lo: the fused head has already handled this bucket's only layer)
    (void)dry_note(n, " bucket %d: layers %d .. %d", k, hi, lo);
    if (hi >= lo) RTRY(backward_layers(n, bw.x, bw.B, 0.f, bw.grad, false, hi, lo, false));
    RTRY(run_reduce_jobs(n, 0.f, false));
    bw.next = hi < lo - 1 ? hi : lo - 1;
    bw.taken = k + 1;
    if (off) *off = bw.off[k];
    if (len) *len = bw.len[k];
    (void)dry_note(n, " bucket %d done: grad[%lld, +%lld) = %.2f MB is final -- its all-reduce may start while the layers below run", k, bw.off[k], bw.len[k], bw.len[k] * 4.0 / 1e6);
    return 0;
}

// the layer table of a net (shapes, padded sizes, parameter offsets) from its description; no device involved
int describe_layers(rcn_hipx_net* n, int in_h, int in_w, int in_c, const rcn_hipx_layer* layers, int n_layers) {
    int H = in_h, W = in_w, C = in_c;
    bool flat = false;
    // "layer i (KIND): " in front of the refusals of a kind that names its layer; the older kinds' refusals stand unprefixed
    auto at_layer = [](int i, int kind) { return kind_row(kind).named ? "layer " + std::to_string(i) + " (" + kind_row(kind).name + "): " : std::string(); };
    for (int i = 0; i < n_layers; ++i) {
        Layer l{};
        l.kind = layers[i].kind; l.H = H; l.W = W; l.Cin = C;
        const int pk = i > 0 ? n->L.back().kind : -1;          // the layer in front (-1: none, a row that is nothing)
        const KindRow &k = l.row(), &prev = kind_row(pk);
        const int out = layers[i].out;
        const std::string at = at_layer(i, l.kind);
        // A bias-only layer must be followed directly by batch normalisation.  For the kinds that name their layer this is said before the
        // next layer's own checks run; for RCN_HIPX_CONV3X3 behind them (below the branches).
        // (RCN_HIPX_DWCONV3X3_S2 says it in a sentence of its own, which names all five batch-normalisation kinds)
        if (pk == RCN_HIPX_DWCONV3X3_S2 && !k.bn)
            return fail(n, -2, at_layer(i - 1, pk) + "it must be followed directly by a batch-normalisation layer (RCN_HIPX_BN_RELU, RCN_HIPX_BN_ADD_RELU, RCN_HIPX_BN_ADD_RELU_DOWN, RCN_HIPX_BN or RCN_HIPX_BN_ADD)");
        if (prev.linear && prev.named && !k.bn) return fail(n, -2, at_layer(i - 1, pk) + "it must be followed directly by a batch-normalisation layer (RCN_HIPX_BN_RELU, RCN_HIPX_BN_ADD_RELU or RCN_HIPX_BN_ADD_RELU_DOWN)");
        // A batch normalisation without a ReLU (RCN_HIPX_BN, RCN_HIPX_BN_ADD) feeds a convolution only: k_pool_bwd folds the mask "pooled value
        // > 0" in, launch_gap_backward gates the layer below, and a dense layer above a batch normalisation leaves it to gate itself -- all
        // three read a batch-normalisation map as a ReLU map.  (A value that is no kind goes on to its own refusal below.)
        if (prev.bn && !prev.relu && !k.map && l.kind >= 0 && l.kind < kKindCount)
            return fail(n, -2, at_layer(i - 1, pk) + "a batch normalisation without a ReLU must be followed directly by a convolution of any kind, not by a " + k.name +
                               " layer (the backward pass of a pool, a global average pool or a dense layer gates for a ReLU below it)");
        if (k.map) {
            // torch.nn.Conv2d(C, out, ks, stride, padding = ks / 2) on the H x W map: a [W | b] block with K = ks * ks * C.  The depthwise one
            // (groups = C): K = 9 and Cout = C, `out` 0 or C (the resolved width is what the state descriptor stores).  Stride 2, pad 1: the
            // output is (H/2) x (W/2), no odd maps in this version.  Only the stride-1 3x3 GEMM kinds have a gather form for a first layer of
            // 9 * Cin <= 32; every other kind's rows are whole 16-byte pieces of a map of a multiple of 32 channels.
            const bool dw = l.kind == RCN_HIPX_DWCONV3X3 || l.kind == RCN_HIPX_DWCONV3X3_S2, conv3 = k.gemm && k.ks == 3;
            if (flat) return fail(n, -2, at + "convolution after a dense layer or a global average pool");
            if (dw && out != 0 && out != C) return fail(n, -2, at + "out must be 0 or the input channels " + std::to_string(C) + " (depth multiplier 1), not " + std::to_string(out));
            if (!dw && (out < 32 || out % 32)) return fail(n, -3, at + "conv output channels must be a positive multiple of 32");
            // (every 3x3 GEMM kind words this one the same way, the strided one too)
            if (conv3 && !(9 * C <= 32) && C % 32) return fail(n, -3, "conv input channels must be a multiple of 32 (or 9*Cin <= 32 for the first layer)");
            if (k.stride == 2 && (H % 2 || W % 2)) return fail(n, -3, at + "a strided convolution needs even height and width, not " + std::to_string(H) + "x" + std::to_string(W));
            if (!(conv3 && k.stride == 1) && C % 32) return fail(n, -3, at + "its input channels must be a multiple of 32, not " + std::to_string(C) + (k.stride == 2 ? " (no strided first-layer form)" : " (no first-layer gather form)"));
            l.Cout = l.CoutP = dw ? C : out; l.oH = H / k.stride; l.oW = W / k.stride; l.K = dw ? 9 : k.ks * k.ks * C;
            H = l.oH; W = l.oW; C = l.Cout;
        } else if (l.kind == RCN_HIPX_MAXPOOL2) {
            if (flat || i == 0 || (pk != RCN_HIPX_CONV3X3_RELU && !prev.bn)) return fail(n, -2, "max-pool must follow a convolution");
            if (H % 2 || W % 2) return fail(n, -3, "max-pool needs even height and width");
            l.Cout = l.CoutP = C; l.oH = H / 2; l.oW = W / 2; l.K = 0;
            n->L.back().pool_follows = true;
            H = l.oH; W = l.oW;
        } else if (l.kind == RCN_HIPX_BN_RELU) {
            if (!prev.linear) return fail(n, -2, "batch normalisation (RCN_HIPX_BN_RELU) must directly follow a RCN_HIPX_CONV3X3 layer (of either stride) or a RCN_HIPX_CONV1X1 layer");
            l.Cout = l.CoutP = C; l.oH = H; l.oW = W; l.K = 1;      // [gamma | beta]: a [W | b] block with K = 1
        } else if (l.kind == RCN_HIPX_BN) {
            // torch.nn.BatchNorm2d(C) and nothing behind it: RCN_HIPX_BN_RELU's block, statistics and buffers
            if (!prev.linear)
                return fail(n, -2, at + "it must directly follow a bias-only convolution (RCN_HIPX_CONV3X3, RCN_HIPX_CONV3X3_S2, RCN_HIPX_CONV1X1, RCN_HIPX_DWCONV3X3 or RCN_HIPX_DWCONV3X3_S2)");
            l.Cout = l.CoutP = C; l.oH = H; l.oW = W; l.K = 1;
        } else if (l.kind == RCN_HIPX_BN_ADD_RELU || l.kind == RCN_HIPX_BN_ADD_RELU_DOWN || l.kind == RCN_HIPX_BN_ADD) {
            // `out` is the distance to the skip's source, the output of layer i - out.  The source needs a gradient buffer that the
            // input-gradient kernel of the layer above it writes in full (backward_layers adds the skip's share behind that launch) and an
            // output that the forward pass writes: a ReLU layer or a pool of this layer's shape, not a convolution whose pool is fused away.
            // RCN_HIPX_BN_ADD_RELU_DOWN: the same, but the source is twice this layer's height and width and may be narrower (option-A shortcut)
            // RCN_HIPX_BN_ADD: RCN_HIPX_BN_ADD_RELU's rules (an identity skip); the two sentences that list kinds are its own
            const bool down = l.kind == RCN_HIPX_BN_ADD_RELU_DOWN, lin = l.kind == RCN_HIPX_BN_ADD;
            if (lin && !prev.linear)
                return fail(n, -2, at + "it must directly follow a bias-only convolution (RCN_HIPX_CONV3X3, RCN_HIPX_CONV3X3_S2, RCN_HIPX_CONV1X1, RCN_HIPX_DWCONV3X3 or RCN_HIPX_DWCONV3X3_S2)");
            if (!prev.linear) return fail(n, -2, at + "it must directly follow a RCN_HIPX_CONV3X3 layer (of either stride) or a RCN_HIPX_CONV1X1 layer");
            if (out < 2) return fail(n, -1, at + "out is the distance to the skip's source and must be at least 2, not " + std::to_string(out));
            const int src = i - out;
            if (src < 0) return fail(n, -2, at + "the skip's source would lie in front of layer 0 (the net's input has no gradient buffer to add into)");
            l.Cout = l.CoutP = C; l.oH = H; l.oW = W; l.K = 1;
            Layer& s = n->L[src];
            const std::string from = at + "the skip's source, layer " + std::to_string(src) + ", ";
            // (a source that is RCN_HIPX_BN or RCN_HIPX_BN_ADD passes for every kind that adds a skip: its share is not gated by the source's output)
            if (lin && s.kind != RCN_HIPX_CONV3X3_RELU && s.kind != RCN_HIPX_MAXPOOL2 && !s.row().bn)
                return fail(n, -2, from + "must be a RCN_HIPX_CONV3X3_RELU or RCN_HIPX_MAXPOOL2 layer or a batch-normalisation layer of any kind (RCN_HIPX_BN_RELU, RCN_HIPX_BN_ADD_RELU, "
                                          "RCN_HIPX_BN_ADD_RELU_DOWN, RCN_HIPX_BN or RCN_HIPX_BN_ADD): a bias-only convolution's map is not yet normalised");
            if (s.kind != RCN_HIPX_CONV3X3_RELU && s.kind != RCN_HIPX_MAXPOOL2 && !s.row().bn)
                return fail(n, -2, from + "must be a RCN_HIPX_CONV3X3_RELU, RCN_HIPX_BN_RELU, RCN_HIPX_BN_ADD_RELU or RCN_HIPX_MAXPOOL2 layer (a RCN_HIPX_CONV3X3 map is not yet normalised)");
            if (s.pool_follows) return fail(n, -2, from + "has a max-pool behind it: its own output is not written when the two fuse -- the source must be the pool");
            if (down) {
                const std::string shape = std::to_string(s.oH) + "x" + std::to_string(s.oW) + "x" + std::to_string(s.CoutP);
                if (s.oH != 2 * l.oH || s.oW != 2 * l.oW)
                    return fail(n, -2, from + "has the output shape " + shape + ": a downsampling shortcut needs exactly twice this layer's " + std::to_string(l.oH) + "x" + std::to_string(l.oW));
                if (s.CoutP > l.CoutP) return fail(n, -2, from + "has more channels (" + std::to_string(s.CoutP) + ") than this layer (" + std::to_string(l.CoutP) + "): the shortcut pads, it does not project");
                if ((l.CoutP - s.CoutP) % 8) return fail(n, -3, from + "leaves " + std::to_string(l.CoutP - s.CoutP) + " channels to pad: (C - Cs) must be a multiple of 8 (the window starts at a multiple of 4)");
            } else if (s.oH != l.oH || s.oW != l.oW || s.CoutP != l.CoutP)
                return fail(n, -2, from + "has another output shape (" + std::to_string(s.oH) + "x" + std::to_string(s.oW) + "x" + std::to_string(s.CoutP) + ", not " +
                                   std::to_string(l.oH) + "x" + std::to_string(l.oW) + "x" + std::to_string(l.CoutP) + "): an identity skip crosses no pool and changes no width");
            if (s.skip_by >= 0) return fail(n, -3, from + "already feeds the skip of layer " + std::to_string(s.skip_by) + ": one skip per source");
            l.skip_src = src; s.skip_by = i;
        } else if (l.kind == RCN_HIPX_GLOBAL_AVGPOOL) {
            // [B][H][W][C] -> [B][C]: the dense stage begins (flat), C unchanged, so the dense layer behind has K = C; no parameter block.  The
            // map in front must be one the forward pass writes in fp32 behind a ReLU or a max-pool (a bare RCN_HIPX_CONV3X3 is refused below)
            if (i == 0) return fail(n, -2, at + "it cannot be the first layer: it pools the map of a convolution, batch normalisation or max-pool layer");
            if (flat) return fail(n, -2, at + "it must follow a map, not a dense layer or another global average pool (layer " + std::to_string(i - 1) + ")");
            if (pk != RCN_HIPX_CONV3X3 && pk != RCN_HIPX_CONV3X3_RELU && pk != RCN_HIPX_MAXPOOL2 && !prev.bn)
                return fail(n, -2, at + "it must directly follow a RCN_HIPX_CONV3X3_RELU, RCN_HIPX_BN_RELU, RCN_HIPX_BN_ADD_RELU or RCN_HIPX_MAXPOOL2 layer");
            l.Cout = l.CoutP = C; l.oH = l.oW = 1; l.K = 0;
            flat = true; H = W = 1;
        } else if (l.kind == RCN_HIPX_DENSE_RELU || l.kind == RCN_HIPX_DENSE) {
            const long long feat = flat ? C : (long long)H * W * C;
            if (feat % 32 || feat > 0x7fffffff) return fail(n, -3, "dense input features must be a multiple of 32");
            if (out < 1) return fail(n, -1, "dense units must be positive");
            if (l.kind == RCN_HIPX_DENSE_RELU && out % 32) return fail(n, -3, "hidden dense units must be a multiple of 32");
            if (l.kind == RCN_HIPX_DENSE && i != n_layers - 1) return fail(n, -2, "the logits layer must be last");
            l.K = (int)feat; l.H = 1; l.W = 1; l.Cin = (int)feat; l.Cout = out; l.CoutP = (l.Cout + 31) / 32 * 32; l.oH = l.oW = 1;
            C = l.Cout; flat = true; H = W = 1;
        } else return fail(n, -1, "unknown layer kind");
        // (RCN_HIPX_CONV3X3 only: behind a kind that names its layer the loop's first check has returned)
        if (prev.linear && !k.bn) return fail(n, -2, "layer " + std::to_string(i - 1) + ": a " + prev.name + " layer must be followed by RCN_HIPX_BN_RELU or RCN_HIPX_BN_ADD_RELU");
        if (k.params) {
            l.w_off = n->n_pad; n->n_pad += (long long)l.K * l.CoutP; l.b_off = n->n_pad; n->n_pad += l.CoutP;
            l.lw_off = n->n_log; n->n_log += (long long)l.K * l.Cout; l.lb_off = n->n_log; n->n_log += l.Cout;
        }
        n->L.push_back(std::move(l));
    }
    const KindRow& last = n->L.back().row();
    if (last.bn && !last.relu)
        return fail(n, -2, at_layer(n_layers - 1, n->L.back().kind) + "a batch normalisation without a ReLU must be followed directly by a convolution of any kind, and the last layer must be RCN_HIPX_DENSE (logits)");
    if (last.linear && last.named) return fail(n, -2, at_layer(n_layers - 1, n->L.back().kind) + "it must be followed directly by a batch-normalisation layer, and the last layer must be RCN_HIPX_DENSE (logits)");
    if (n->L.back().kind != RCN_HIPX_DENSE) return fail(n, -2, "the last layer must be RCN_HIPX_DENSE (logits)");
    n->classes = n->L.back().Cout;
    // one reduction launch, and one state pack, take kMaxReduceJobs layers with parameters: refused here, so create, every plan and the
    // state layout agree before anything is enqueued (reduce_slab and make_state_jobs keep their own guards)
    int with_params = 0;
    for (const Layer& l : n->L) with_params += l.row().params;
    if (with_params > kMaxReduceJobs)
        return fail(n, -3, std::to_string(with_params) + " layers with parameters: one reduction launch and one state pack take at most " + std::to_string(kMaxReduceJobs));
    return 0;
}

// the layer descriptions of `from` without their buffers (host-only dry-run nets)
void copy_layer_table(rcn_hipx_net& to, const rcn_hipx_net& from) {
    for (const Layer& l : from.L) { to.L.emplace_back(); static_cast<LayerShape&>(to.L.back()) = l; }
    to.n_pad = from.n_pad; to.n_log = from.n_log;
}

// Host-only nets for dry runs (no device, no stream, no buffers).  From a description: what rcn_hipx_create would make of it now (options
// seeded from the environment), `mode` being a rcn_hipx_set_precision mode; returns describe_layers' status ...
int make_dry_net(rcn_hipx_net& net, int in_h, int in_w, int in_c, const rcn_hipx_layer* layers, int n_layers, int batch, int mode, int tiling) {
    net.in_h = in_h; net.in_w = in_w; net.in_c = in_c; net.max_batch = batch; net.dry = true;
    net.precision = mode == RCN_HIPX_FP32 ? RCN_HIPX_FP32 : RCN_HIPX_BF16; net.store16 = mode == RCN_HIPX_BF16_STORED; net.tiling = tiling;
    seed_options(net.opt);
    return describe_layers(&net, in_h, in_w, in_c, layers, n_layers);
}
// ... or from an existing net: its layers, precision, tiling, options, optimiser, loss, average, clipping, accumulation and dropout -- the plan and the step agree by construction
void make_dry_net(rcn_hipx_net& net, const rcn_hipx_net& from, int batch) {
    net.in_h = from.in_h; net.in_w = from.in_w; net.in_c = from.in_c; net.max_batch = batch; net.classes = from.classes; net.dry = true;
    static_cast<Selection&>(net) = from;
    static_cast<Recipe&>(net) = from;
    copy_layer_table(net, from);
}

// Would every layer of this net run on kernels that take bf16 tensors (RCN_HIPX_BF16_STORED)?  Asked of the plan, the same walk as the step
// at the net's largest batch: 0, or the step's status with its message in *why.
int store16_covered(const rcn_hipx_net& n, std::string* why) {
    rcn_hipx_net probe;
    make_dry_net(probe, n, n.max_batch);
    probe.precision = RCN_HIPX_BF16; probe.store16 = true;
    const int st = step_core(&probe, nullptr, nullptr, n.max_batch, 0.f, nullptr, true, nullptr);
    if (st != 0) *why = probe.err;
    return st;
}

const char* precision_name(int precision, bool store16) { return precision != RCN_HIPX_BF16 ? "fp32 operands" : store16 ? "bf16 operands, the convolutional stage's tensors stored as bf16" : "bf16 operands"; }

// ---- the plans' shared pieces
// the arguments every plan of a description shares
bool plan_args_ok(int in_h, int in_w, int in_c, const rcn_hipx_layer* layers, int n_layers, int batch, int precision, int tiling, const char* out, int cap) {
    return layers && n_layers >= 1 && in_h >= 1 && in_w >= 1 && in_c >= 1 && batch >= 1 && out && cap >= 1 &&
           (precision == RCN_HIPX_FP32 || precision == RCN_HIPX_BF16 || precision == RCN_HIPX_BF16_STORED) && tiling >= RCN_HIPX_TILING_GEMM && tiling <= RCN_HIPX_TILING_LDS;
}
// the sentence in front of a training step's launches
std::string step_header(const rcn_hipx_net& net, int batch) {
    return "forward + loss + backward of one batch of " + std::to_string(batch) + " (" + precision_name(net.precision, net.store16) + "), launch by launch:\n";
}
// a dry walk's text, or why it stopped, into the caller's buffer; returns the walk's status
int emit(const rcn_hipx_net& net, int st, char* out, int cap) {
    std::snprintf(out, (size_t)cap, "%s", (st == 0 ? net.plan : net.err).c_str());
    return st;
}

}  // namespace

extern "C" {

int rcn_hipx_create(int device, int in_h, int in_w, int in_c, const rcn_hipx_layer* layers, int n_layers, int max_batch, void* stream, rcn_hipx_net** out) {
    if (!out || !layers || n_layers < 1 || in_h < 1 || in_w < 1 || in_c < 1 || max_batch < 1) return -1;
    *out = nullptr;
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || device < 0 || device >= ndev) return -5;
    rcn_hipx_net* n = new (std::nothrow) rcn_hipx_net();
    if (!n) return -7;
    *out = n;
    n->device = device; n->in_h = in_h; n->in_w = in_w; n->in_c = in_c; n->max_batch = max_batch;
    n->tiling = halo_f32_default();
    seed_options(n->opt);                             // the environment seeds the defaults, once, here
    RTRY(describe_layers(n, in_h, in_w, in_c, layers, n_layers));
    Dev g(device);
    if (stream) { n->stream = (hipStream_t)stream; } else { XTRY(n, hipStreamCreateWithFlags(&n->stream, hipStreamNonBlocking)); n->own_stream = true; }
    { const char* e = std::getenv("RCN_HIPX_OVERLAP"); n->overlap = e ? std::atoi(e) : 0; }
    XTRY(n, hipStreamCreateWithFlags(&n->side, hipStreamNonBlocking));
    XTRY(n, n->params.ensure((size_t)n->n_pad * sizeof(float)));
    XTRY(n, hipMemsetAsync(n->params.p, 0, (size_t)n->n_pad * sizeof(float), n->stream));
    XTRY(n, n->wt.ensure((size_t)n->n_pad * sizeof(float)));
    XTRY(n, hipMemsetAsync(n->wt.p, 0, (size_t)n->n_pad * sizeof(float), n->stream));
    for (Layer& l : n->L) {
        const size_t elems = (size_t)max_batch * l.oH * l.oW * l.CoutP;
        XTRY(n, l.out.ensure(elems * sizeof(float)));
        XTRY(n, l.dout.ensure(elems * sizeof(float)));
        if (l.kind == RCN_HIPX_MAXPOOL2) XTRY(n, l.idx.ensure(elems));
        if (l.row().bn) {
            XTRY(n, l.bn.ensure((size_t)4 * l.CoutP * sizeof(float)));
            XTRY(n, l.bn_part.ensure((size_t)bn_parts_cap((long long)max_batch * l.oH * l.oW) * 2 * l.CoutP * sizeof(double)));
            XTRY(n, l.slab.ensure((size_t)2 * l.CoutP * sizeof(float)));
        }
    }
    RTRY(bn_reset_stats(n));
    XTRY(n, hipStreamSynchronize(n->stream));
    return 0;
}

void rcn_hipx_destroy(rcn_hipx_net* n) {
    if (!n) return;
    Dev g(n->device);
    if (n->stream) (void)hipStreamSynchronize(n->stream);
    drop_graphs(n);
    if (n->side) { (void)hipStreamSynchronize(n->side); (void)hipStreamDestroy(n->side); }
    for (hipEvent_t e : n->events) (void)hipEventDestroy(e);
    if (n->own_stream && n->stream) (void)hipStreamDestroy(n->stream);
    delete n;                                           // every Buf frees its memory here: the device current, the streams drained
}

const char* rcn_hipx_last_error(const rcn_hipx_net* n) { return n ? n->err.c_str() : "null net"; }
int rcn_hipx_synchronize(rcn_hipx_net* n) { if (!n) return -1; Dev g(n->device); XTRY(n, hipStreamSynchronize(n->stream)); return 0; }
int rcn_hipx_param_count(const rcn_hipx_net* n, int64_t* logical, int64_t* padded) { if (!n) return -1; if (logical) *logical = n->n_log; if (padded) *padded = n->n_pad; return 0; }
int rcn_hipx_classes(const rcn_hipx_net* n) { return n ? n->classes : -1; }

int rcn_hipx_set_precision(rcn_hipx_net* n, int mode) {
    if (!n) return -1;
    if (mode != RCN_HIPX_FP32 && mode != RCN_HIPX_BF16 && mode != RCN_HIPX_BF16_STORED)
        return fail(n, -1, "set_precision: mode must be RCN_HIPX_FP32, RCN_HIPX_BF16 or RCN_HIPX_BF16_STORED");
    const int prec = mode == RCN_HIPX_FP32 ? RCN_HIPX_FP32 : RCN_HIPX_BF16;
    const bool st16 = mode == RCN_HIPX_BF16_STORED;
    if (st16) {                                         // before anything changes
        std::string why;
        const int ps = store16_covered(*n, &why);
        if (ps != 0) return fail(n, ps, why);
    }
    Dev g(n->device);
    if (prec != n->precision || st16 != n->store16) { XTRY(n, hipStreamSynchronize(n->stream)); drop_graphs(n); }
    n->precision = prec;
    n->store16 = st16;
    return 0;
}

int rcn_hipx_set_tiling(rcn_hipx_net* n, int mode) {
    if (!n) return -1;
    if (mode != RCN_HIPX_TILING_GEMM && mode != RCN_HIPX_TILING_AUTO && mode != RCN_HIPX_TILING_LDS) return fail(n, -1, "set_tiling: unknown mode");
    Dev g(n->device);
    if (mode != n->tiling) { XTRY(n, hipStreamSynchronize(n->stream)); drop_graphs(n); }
    n->tiling = mode;
    return 0;
}

int rcn_hipx_set_overlap(rcn_hipx_net* n, int on) {
    if (!n) return -1;
    Dev g(n->device);
    if (on != n->overlap) { XTRY(n, hipStreamSynchronize(n->stream)); drop_graphs(n); }
    n->overlap = on;
    return 0;
}

int rcn_hipx_set_option(rcn_hipx_net* n, const char* name, int value) {
    if (!n || !name) return -1;
    for (const XOptDesc& d : kXOptTable)
        if (std::strcmp(d.name, name) == 0) {
            if (value < d.lo || value > d.hi) return fail(n, -1, std::string("set_option: ") + name + " must be in " + std::to_string(d.lo) + ".." + std::to_string(d.hi));
            if (n->opt.*(d.field) == value) return 0;
            Dev g(n->device);
            XTRY(n, hipStreamSynchronize(n->stream));
            drop_graphs(n);                             // captured graphs bake in the kernels chosen
            n->opt.*(d.field) = value;
            return 0;
        }
    return fail(n, -1, std::string("set_option: unknown option '") + name + "'");
}

int rcn_hipx_get_option(const rcn_hipx_net* n, const char* name, int* value) {
    if (!n || !name || !value) return -1;
    for (const XOptDesc& d : kXOptTable)
        if (std::strcmp(d.name, name) == 0) { *value = n->opt.*(d.field); return 0; }
    return -1;
}

// a flat logical array (rcn_hipx_get_params' layout) into a padded buffer of the net, the padding zero; unpad is its inverse.  Returns
// with the copy done: the staging array must outlive it.
static int upload_padded(rcn_hipx_net* n, Buf& to, const float* flat) {
    std::vector<float> pad((size_t)n->n_pad, 0.f);
    for (const Layer& l : n->L) {
        if (!l.row().params) continue;
        for (int k = 0; k < l.K; ++k) std::memcpy(&pad[l.w_off + (long long)k * l.CoutP], &flat[l.lw_off + (long long)k * l.Cout], sizeof(float) * l.Cout);
        std::memcpy(&pad[l.b_off], &flat[l.lb_off], sizeof(float) * l.Cout);
    }
    XTRY(n, hipMemcpyAsync(to.p, pad.data(), pad.size() * sizeof(float), hipMemcpyHostToDevice, n->stream));
    XTRY(n, hipStreamSynchronize(n->stream));
    return 0;
}

int rcn_hipx_set_params(rcn_hipx_net* n, const float* flat) {
    if (!n || !flat) return -1;
    Dev g(n->device);
    RTRY(upload_padded(n, n->params, flat));
    RTRY(refresh_flipped(n));
    XTRY(n, hipStreamSynchronize(n->stream));
    return 0;
}

static int unpad(rcn_hipx_net* n, const float* dev, float* flat) {
    std::vector<float> pad((size_t)n->n_pad);
    XTRY(n, hipMemcpyAsync(pad.data(), dev, pad.size() * sizeof(float), hipMemcpyDeviceToHost, n->stream));
    XTRY(n, hipStreamSynchronize(n->stream));
    for (const Layer& l : n->L) {
        if (!l.row().params) continue;
        for (int k = 0; k < l.K; ++k) std::memcpy(&flat[l.lw_off + (long long)k * l.Cout], &pad[l.w_off + (long long)k * l.CoutP], sizeof(float) * l.Cout);
        std::memcpy(&flat[l.lb_off], &pad[l.b_off], sizeof(float) * l.Cout);
    }
    return 0;
}

int rcn_hipx_get_params(rcn_hipx_net* n, float* flat) { if (!n || !flat) return -1; Dev g(n->device); return unpad(n, (const float*)n->params.p, flat); }
int rcn_hipx_unpad_host(rcn_hipx_net* n, const float* padded_dev, float* logical_host) { if (!n || !padded_dev || !logical_host) return -1; Dev g(n->device); return unpad(n, padded_dev, logical_host); }

int rcn_hipx_init_params(rcn_hipx_net* n, uint64_t seed) {
    if (!n) return -1;
    std::mt19937_64 gen(seed ? seed : std::random_device{}());
    std::vector<float> flat((size_t)n->n_log, 0.f);
    for (const Layer& l : n->L) {
        if (!l.row().params) continue;
        if (l.row().bn) { for (int c = 0; c < l.Cout; ++c) flat[l.lw_off + c] = 1.f; continue; }      // gamma = 1, beta = 0
        std::normal_distribution<float> nd(0.f, std::sqrt(2.0f / (float)l.K));
        for (long long i = 0; i < (long long)l.K * l.Cout; ++i) flat[l.lw_off + i] = nd(gen);
    }
    return rcn_hipx_set_params(n, flat.data());
}

int rcn_hipx_forward_dev(rcn_hipx_net* n, const float* x, int B, float* logits) {
    if (!n || !x || !logits) return -1;
    RTRY(ensure_batch(n, B));
    Dev g(n->device);
    RTRY(prep_bf16_weights(n));
    RTRY(forward(n, x, B));
    const Layer& l = n->L.back();
    XTRY(n, hipMemcpy2DAsync(logits, (size_t)n->classes * sizeof(float), l.out.p, (size_t)l.CoutP * sizeof(float), (size_t)n->classes * sizeof(float), (size_t)B,
                             hipMemcpyDeviceToDevice, n->stream));
    return 0;
}

// the B logits rows the LAST forward pass left in the last layer's output -- a training step's, a gradients call's or an evaluation's
int rcn_hipx_last_logits_dev(rcn_hipx_net* n, int B, float* logits) {
    if (!n || !logits) return -1;
    RTRY(ensure_batch(n, B));
    if (B != n->last_rows) return fail(n, -6, n->last_rows ? "last_logits: the last forward pass ran another batch size" : "last_logits: no forward pass has run yet");
    Dev g(n->device);
    const Layer& l = n->L.back();
    XTRY(n, hipMemcpy2DAsync(logits, (size_t)n->classes * sizeof(float), l.out.p, (size_t)l.CoutP * sizeof(float), (size_t)n->classes * sizeof(float), (size_t)B,
                             hipMemcpyDeviceToDevice, n->stream));
    return 0;
}

// One eager step (it sizes every scratch buffer outside capture: hipMalloc is illegal while capturing -- and it IS the caller's step),
// then the same step captured and instantiated for the replays that follow.
// *enqueued (nullable) is set once the caller's step is on the stream, whatever becomes of its capture.
static int step_and_capture(rcn_hipx_net* n, const StepKey& k, hipGraphExec_t* exec_out, bool* enqueued = nullptr) {
    const Pair pair{k.labels_b, k.weight};
    RTRY(step_core(n, k.x, k.labels, k.B, k.lr, nullptr, true, k.loss, k.lr_dev, pair, k.micro));
    if (enqueued) *enqueued = true;
    hipGraph_t graph = nullptr;
    XTRY(n, hipStreamBeginCapture(n->stream, hipStreamCaptureModeThreadLocal));
    const int st = step_core(n, k.x, k.labels, k.B, k.lr, nullptr, true, k.loss, k.lr_dev, pair, k.micro);
    hipError_t e = hipStreamEndCapture(n->stream, &graph);
    if (st != 0) { if (graph) (void)hipGraphDestroy(graph); return st; }
    XTRY(n, e);
    hipGraphExec_t exec = nullptr;
    e = hipGraphInstantiate(&exec, graph, nullptr, nullptr, 0);
    (void)hipGraphDestroy(graph);
    XTRY(n, e);
    ++n->n_instantiated;
    *exec_out = exec;
    return 0;
}

// which of the net's caches a step belongs to: on the caller's pointers (plain 0, pair labels 1), or on the net's own batch buffer with
// its rate from the host (2, mixed 3) or from the device (4, mixed 5)
// (a first or middle micro-step of an accumulating net has no lr_dev: it sits with the host-rate steps of its buffers)
static int family_of(const rcn_hipx_net* n, const StepKey& k) { return (k.x != n->xb.p ? 0 : k.lr_dev ? 4 : 2) + (k.labels_b ? 1 : 0); }
static_assert(rcn_hipx_net::kFamilies == 6, "family_of hands out 0 .. 5");

// One training step through the cache: a replay of the graph captured for `key`, or -- at its first use -- the eager step (which IS the
// caller's step) and its capture.  Looked up per step: the eager step of a first use can grow a scratch buffer, which drops every graph.
// *enqueued (nullable): the step itself is on the stream -- true on success, and also where only the capture behind the eager step failed.
static int captured_step(rcn_hipx_net* n, const StepKey& key, bool* enqueued = nullptr) {
    auto& graphs = n->graphs[family_of(n, key)];
    auto it = graphs.find(key);
    if (it != graphs.end()) { XTRY(n, hipGraphLaunch(it->second, n->stream)); if (enqueued) *enqueued = true; return 0; }
    hipGraphExec_t exec = nullptr;
    RTRY(step_and_capture(n, key, &exec, enqueued));
    if (graphs.size() >= 8) drop_all(graphs);           // (eight keys: a caller that varies lr per call)
    graphs.emplace(key, exec);
    return 0;
}

// which micro-step the next training step of the net is (kWholeStep: the net does not accumulate)
static int next_micro(const rcn_hipx_net* n) {
    if (n->accum_k == 1) return kWholeStep;
    return n->accum_pos == 0 ? kMicroFirst : n->accum_pos == n->accum_k - 1 ? kMicroLast : kMicroMiddle;
}

// One training step of a net that may accumulate: the step `key` describes as the micro-step the net's position in its cycle makes it.
// Only the micro-step that applies the update keeps the key's rate.  The position advances once the micro-step is on the stream: a first use
// runs the step eagerly and then captures it, and a failure of that capture must not leave the position behind the accumulator (a retry
// would add the batch twice).  A step that fails before its reduction launch has changed neither.
static int training_step(rcn_hipx_net* n, StepKey key) {
    key.micro = next_micro(n);
    if (key.micro == kMicroFirst || key.micro == kMicroMiddle) { key.lr = 0.f; key.lr_dev = nullptr; }
    bool enqueued = false;
    const int st = captured_step(n, key, &enqueued);
    if (enqueued && key.micro != kWholeStep) n->accum_pos = (n->accum_pos + 1) % n->accum_k;
    return st;
}

int rcn_hipx_train_step_dev(rcn_hipx_net* n, const float* x, const int32_t* labels, int B, float lr, float* loss_dev) {
    if (!n || !x || !labels) return -1;
    RTRY(ensure_batch(n, B));
    Dev g(n->device);
    n->walk_open = false;                               // (a step in between abandons an open bucket walk's activations)
    return training_step(n, StepKey{x, labels, nullptr, nullptr, B, lr, nullptr, loss_dev});
}

int rcn_hipx_train_step_pair_dev(rcn_hipx_net* n, const float* x, const int32_t* labels_a, const int32_t* labels_b, const float* weight, int B, float lr, float* loss_dev) {
    if (!n || !x || !labels_a || !labels_b) return -1;
    RTRY(ensure_batch(n, B));
    Dev g(n->device);
    n->walk_open = false;
    return training_step(n, StepKey{x, labels_a, labels_b, weight, B, lr, nullptr, loss_dev});
}

// ---- the loop around the step: an epoch over a device-resident set, and evaluation --------------------------------------------------------
namespace {

bool x_kind_ok(int k) { return k == RCN_HIPX_X_F32 || k == RCN_HIPX_X_U8; }
long long row_elems(const rcn_hipx_net* n) { return (long long)n->in_h * n->in_w * n->in_c; }

// the net's own batch, labels and loss buffers: sized for max_batch once, so they never move under a captured graph
int ensure_epoch_bufs(rcn_hipx_net* n) {
    XTRY(n, n->xb.ensure((size_t)n->max_batch * row_elems(n) * sizeof(float)));
    XTRY(n, n->yb.ensure((size_t)n->max_batch * sizeof(int32_t)));
    XTRY(n, n->eloss.ensure(sizeof(float)));
    XTRY(n, n->elr.ensure(sizeof(float)));
    return 0;
}
// ... and, for mixed samples, the partners' labels and the target weight
int ensure_mix_bufs(rcn_hipx_net* n) {
    XTRY(n, n->yb2.ensure((size_t)n->max_batch * sizeof(int32_t)));
    XTRY(n, n->emixw.ensure(sizeof(float)));
    return 0;
}
static_assert(sizeof(rcn_hipx_mix_step) == 24 && sizeof(MixStep) == 24 && offsetof(rcn_hipx_mix_step, y0) == offsetof(MixStep, y0), "MixStep is rcn_hipx_mix_step");

// nullptr, or why this rcn_hipx_augment is refused for a net of this input shape (H = W = 0: the shape-free part, for the host draw)
const char* augment_refusal(const rcn_hipx_augment* a, int H, int W) {
    if (a->pad < 0 || a->pad > 16) return "augment: pad must be in 0 .. 16";
    if (H > 0 && a->pad >= (H < W ? H : W)) return "augment: pad must be smaller than the image's height and width";
    if (a->hflip != 0 && a->hflip != 1) return "augment: hflip must be 0 or 1";
    return nullptr;
}

// rows idx[0 .. B) (idx == NULL: base .. base + B - 1) of the set into dst ([B][row] fp32), their labels (nullable) into ydst; aug
// (nullable): through the augmentation, row r drawing with q0 + r.  mix (nullable; one record on the device): mixed with the mirrored row
// of the batch, whose labels go to ydst_b.  The launch is select_gather's (convnet_epoch.hpp).
int launch_gather(rcn_hipx_net* n, const void* X, int x_kind, float x_scale, float x_shift, const int32_t* labels, long long rows, const int32_t* idx, long long base, int B,
                  const rcn_hipx_augment* aug, unsigned long long q0, float* dst, int* ydst, const rcn_hipx_mix_step* mix = nullptr, int* ydst_b = nullptr) {
    const int E = (int)row_elems(n);
    const RowScale rs{x_scale, x_shift};
    const bool u8 = x_kind == RCN_HIPX_X_U8;
    const bool dry = n->dry;                            // (a plan: the set and the batch buffer are taken to be aligned, as allocators return them)
    const GatherChoice c = select_gather(u8, B, E, dry || (uintptr_t)X % 16 == 0, dry || (uintptr_t)dst % 16 == 0, aug != nullptr, mix != nullptr);
    if (!c.blocks) return fail(n, -3, "a batch of more than 2^37 elements");
    const AugSpec as = aug ? AugSpec{aug->seed, aug->epoch, aug->pad, aug->hflip} : AugSpec{0, 0, 0, 0};
    const dim3 grid((unsigned)c.blocks), block(kGatherThreads);
    const int H = n->in_h, W = n->in_w, Cc = n->in_c;
    if (mix) {
        char augtext[48] = "no augmentation";
        if (aug) std::snprintf(augtext, sizeof augtext, "augment pad %d hflip %d", (int)aug->pad, (int)aug->hflip);
        if (dry_note(n, "  gather: k_gather_mix<%s, %d>, %s, %lld workgroups, partner row B - 1 - r, %s", u8 ? "uint8" : "float", c.vec,
                     c.vec == 4 ? "one or two source elements per output, 16-byte stores" : "element by element", c.blocks, augtext)) return 0;
        with_row_type(u8, [&](auto T) { with_const<4, 1>(c.vec, [&](auto VEC) {
            hipLaunchKernelGGL((k_gather_mix<CT(T), CV(VEC)>), grid, block, 0, n->stream, (const CT(T)*)X, labels, rows, idx, base, B, H, W, Cc, rs, aug ? 1 : 0, as, q0,
                               reinterpret_cast<const MixStep*>(mix), dst, ydst, ydst_b);
        }); });
    } else if (aug) {
        if (dry_note(n, "  gather: k_gather_aug<%s, %d>, %s, %lld workgroups, augment pad %d hflip %d", u8 ? "uint8" : "float", c.vec,
                     c.vec == 4 ? "one source element per output, 16-byte stores" : "element by element", c.blocks, (int)aug->pad, (int)aug->hflip)) return 0;
        with_row_type(u8, [&](auto T) { with_const<4, 1>(c.vec, [&](auto VEC) {
            hipLaunchKernelGGL((k_gather_aug<CT(T), CV(VEC)>), grid, block, 0, n->stream, (const CT(T)*)X, labels, rows, idx, base, B, H, W, Cc, rs, as, q0, dst, ydst);
        }); });
    } else {
        if (dry_note(n, "  gather: k_gather_rows<%s, %d>, %s, %lld workgroups", u8 ? "uint8" : "float", c.vec, c.vec > 1 ? "16-byte loads and stores" : "element by element", c.blocks)) return 0;
        with_row_type(u8, [&](auto T) { with_bool(c.vec > 1, [&](auto PIECES) {
            hipLaunchKernelGGL((k_gather_rows<CT(T), CV(PIECES) ? RowPiece<CT(T)>::kVec : 1>), grid, block, 0, n->stream, (const CT(T)*)X, labels, rows, idx, base, B, E, rs, dst, ydst);
        }); });
    }
    XTRY(n, hipGetLastError());
    return 0;
}
#undef CT
#undef CV

// what a metrics call asked for, in the words of its plan line
void metrics_asked(const rcn_hipx_eval_out& o, std::string& t) {
    if (o.n_topk > 0) t += "; top-k counts for " + std::to_string(o.n_topk) + (o.n_topk == 1 ? " k" : " ks");
    if (o.confusion) t += "; confusion matrix";
    if (o.loss_each || o.rank) t += "; per-row loss and rank";
    if (o.logits) t += "; logits copy";
}

// loss sum, correct count and arg-max of the B logits rows the forward pass has just left in the last layer's output; with `o` (a metrics
// call's outputs; the chunk's rows begin at row `off` of them) also what it asks for, in the same launch
int launch_eval(rcn_hipx_net* n, const int32_t* labels, int B, double* loss_sum, long long* correct, int32_t* pred, const rcn_hipx_eval_out* o, int64_t off) {
    const int blocks = eval_blocks(B);
    if (n->dry && o) {
        std::string asked;
        metrics_asked(*o, asked);
        dry_note(n, "  eval: k_eval_metrics, %d workgroups (loss sum, correct count, first-maximum arg-max%s; no gradient)", blocks, asked.c_str());
        return 0;
    }
    if (dry_note(n, "  eval: k_eval_ce, %d workgroups (loss sum, correct count, first-maximum arg-max; no gradient)", blocks)) return 0;
    const Layer& l = n->L.back();
    const size_t parts = (size_t)eval_blocks(n->max_batch);
    if (!n->eval_part.p) {
        XTRY(n, n->eval_part.ensure(((2 + kEvalMaxTopk) * parts + 1) * sizeof(float)));
        XTRY(n, hipMemsetAsync(n->eval_part.p, 0, n->eval_part.cap, n->stream));
    }
    float* const lp = (float*)n->eval_part.p;
    // the plain kernel, or the metrics one with its one trailing argument
    auto launch = [&](auto kernel, auto... metrics) {
        hipLaunchKernelGGL(kernel, dim3(blocks), dim3(256), 0, n->stream, (const float*)l.out.p, labels, B, n->classes, l.CoutP, lp, (int*)(lp + parts), (unsigned*)(lp + 2 * parts),
                           loss_sum, correct, pred, metrics...);
    };
    if (o) {
        const long long C = n->classes;
        EvalMetrics m{};
        m.n_topk = labels ? o->n_topk : 0;
        for (int j = 0; j < m.n_topk; ++j) m.topk[j] = o->topk[j];
        m.topk_part = (int*)(lp + 2 * parts + 1);
        m.part_stride = (int)parts;
        m.topk_correct = (long long*)o->topk_correct;
        m.confusion = (long long*)o->confusion;
        m.loss_each = o->loss_each ? o->loss_each + off : nullptr;
        m.rank = o->rank ? o->rank + off : nullptr;
        m.logits_out = o->logits ? o->logits + off * C : nullptr;
        launch(k_eval<true, EvalMetrics>, m);
    } else {
        launch(k_eval<false>);
    }
    XTRY(n, hipGetLastError());
    return 0;
}

// one evaluation chunk: the forward pass over all layers (rcn_hipx_forward_dev's) and the evaluation kernel
int eval_chunk(rcn_hipx_net* n, const float* x, const int32_t* labels, int B, double* loss_sum, long long* correct, int32_t* pred, const rcn_hipx_eval_out* metrics = nullptr,
               int64_t off = 0) {
    RTRY(forward(n, x, B));
    return launch_eval(n, labels, B, loss_sum, correct, pred, metrics, off);
}

// params <-> average, on the net's stream
int launch_ema_swap(rcn_hipx_net* n) {
    hipLaunchKernelGGL(k_swap4, dim3(grid1d(n->n_pad / 4, 256)), dim3(256), 0, n->stream, (float*)n->params.p, (float*)n->ema.p, n->n_pad);
    XTRY(n, hipGetLastError());
    return 0;
}
// An evaluation on the average: once the first exchange is enqueued, the second one is enqueued on EVERY way out of the scope -- an error in
// a chunk must not leave the net training on the average.  (net == nullptr: the live parameters, nothing to do.)
struct EmaSwap {
    rcn_hipx_net* net;
    bool armed = false;
    int begin() { if (!net) return 0; RTRY(launch_ema_swap(net)); armed = true; return 0; }
    ~EmaSwap() { if (armed) (void)launch_ema_swap(net); }
};

int plan_eval_walk(rcn_hipx_net& net, int batch, const rcn_hipx_eval_out* metrics = nullptr) {
    net.plan = "forward + evaluation of one chunk of " + std::to_string(batch) + " rows (" + precision_name(net.precision, net.store16) + "), launch by launch:\n";
    RTRY(prep_bf16_weights(&net));
    return eval_chunk(&net, nullptr, nullptr, batch, nullptr, nullptr, nullptr, metrics);
}

// why a metrics call's requests are refused (nullptr: they are not); what rcn_hipx_evaluate_ex_dev checks is left to the shared path
const char* metrics_refusal(const rcn_hipx_eval_out* o, int classes, bool with_labels) {
    if (!o) return "out must not be NULL";
    if (o->n_topk < 0 || o->n_topk > RCN_HIPX_EVAL_MAX_TOPK) return "n_topk must lie in 0 .. RCN_HIPX_EVAL_MAX_TOPK";
    for (int j = 0; j < o->n_topk; ++j)
        if (o->topk[j] < 1 || o->topk[j] > classes || (j > 0 && o->topk[j] <= o->topk[j - 1])) return "topk must be strictly increasing with 1 <= k <= classes";
    if (o->n_topk > 0 && !o->topk_correct) return "with n_topk > 0, topk_correct must not be NULL";
    if (!with_labels && (o->n_topk > 0 || o->topk_correct || o->confusion || o->loss_each || o->rank))
        return "without labels only pred and logits can be filled: topk_correct, confusion, loss_each and rank must not be asked for";
    return nullptr;
}

// rcn_hipx_evaluate_ex_dev and rcn_hipx_evaluate_metrics_dev (`metrics`: its outputs, already found in order; loss_sum, correct and pred are
// its first three): the refusals, the zeroing of the accumulators, the exchange with the average, the operand copies and the chunk loop
int evaluate_rows(rcn_hipx_net* n, const void* X, int x_kind, float x_scale, float x_shift, const int32_t* labels, int64_t rows, int weights,
                  double* loss_sum, int64_t* correct, int32_t* pred, const rcn_hipx_eval_out* metrics) {
    if (weights != RCN_HIPX_WEIGHTS_LIVE && weights != RCN_HIPX_WEIGHTS_EMA) return fail(n, -1, "evaluate: weights must be RCN_HIPX_WEIGHTS_LIVE or RCN_HIPX_WEIGHTS_EMA");
    if (!X) return fail(n, -1, "evaluate: X_dev must not be NULL");
    if (!x_kind_ok(x_kind)) return fail(n, -1, "evaluate: x_kind must be RCN_HIPX_X_F32 or RCN_HIPX_X_U8");
    if (rows < 1) return fail(n, -1, "evaluate: n must be at least 1");
    if (labels && (!loss_sum || !correct)) return fail(n, -1, "evaluate: with labels, loss_sum_dev and correct_dev must not be NULL");
    if (!labels && !pred && !(metrics && metrics->logits)) return fail(n, -1, "evaluate: without labels there is only pred_dev to fill; it must not be NULL");
    if (n->walk_open) return fail(n, -6, "evaluate: a bucket walk is open (rcn_hipx_gradients_begin_dev): its activations are still needed; take the remaining buckets first");
    if (weights == RCN_HIPX_WEIGHTS_EMA && !n->ema.p) return fail(n, -6, "evaluate: the net has no average (rcn_hipx_set_ema with a decay > 0 first)");
    Dev g(n->device);
    if (x_kind == RCN_HIPX_X_U8) RTRY(ensure_epoch_bufs(n));
    if (loss_sum) XTRY(n, hipMemsetAsync(loss_sum, 0, sizeof(double), n->stream));
    if (correct) XTRY(n, hipMemsetAsync(correct, 0, sizeof(int64_t), n->stream));
    if (metrics && metrics->n_topk > 0) XTRY(n, hipMemsetAsync(metrics->topk_correct, 0, (size_t)metrics->n_topk * sizeof(int64_t), n->stream));
    if (metrics && metrics->confusion) XTRY(n, hipMemsetAsync(metrics->confusion, 0, (size_t)n->classes * n->classes * sizeof(int64_t), n->stream));
    // On the average: the parameter buffer and the average trade contents for the length of the call, so every pointer the forward pass and
    // k_prep_all_bf16 hold (prep jobs, layer offsets) stays what it is.  The forward pass reads the parameters and, in bf16 mode, the
    // operand copies that the prep launch below makes from them; it never reads the tap-flipped copy `wt` (only the input-gradient pass,
    // the fused training head and the prep job of the input-gradient operand do), so wt is left alone and matches the live parameters
    // again once they are back.  The bf16 operand copies are re-made by the next step, as by every step.
    EmaSwap swapped{weights == RCN_HIPX_WEIGHTS_EMA ? n : nullptr};
    RTRY(swapped.begin());
    RTRY(prep_bf16_weights(n));
    const long long E = row_elems(n);
    for (int64_t off = 0; off < rows; off += n->max_batch) {
        const int B = (int)(rows - off < n->max_batch ? rows - off : n->max_batch);
        const float* x = (const float*)X + off * E;
        if (x_kind == RCN_HIPX_X_U8) {
            RTRY(launch_gather(n, X, x_kind, x_scale, x_shift, nullptr, (long long)rows, nullptr, (long long)off, B, nullptr, 0, (float*)n->xb.p, (int*)n->yb.p));
            x = (const float*)n->xb.p;
        }
        RTRY(eval_chunk(n, x, labels ? labels + off : nullptr, B, loss_sum, (long long*)correct, pred ? pred + off : nullptr, metrics, off));
    }
    return 0;
}

}  // namespace

int rcn_hipx_train_epoch_mix_dev(rcn_hipx_net* n, const void* X, int x_kind, float x_scale, float x_shift, const int32_t* labels, int64_t rows, const int32_t* perm,
                                 int B, int64_t first_batch, int64_t n_batches, float lr, const float* lr_dev, const rcn_hipx_augment* aug, const rcn_hipx_mix_step* mix_dev,
                                 float* loss_dev) {
    if (!n) return -1;
    if (!X || !labels) return fail(n, -1, "train_epoch: X_dev and labels_dev must not be NULL");
    if (!x_kind_ok(x_kind)) return fail(n, -1, "train_epoch: x_kind must be RCN_HIPX_X_F32 or RCN_HIPX_X_U8");
    RTRY(ensure_batch(n, B));
    if (rows < 1 || first_batch < 0 || n_batches < 0 || first_batch > rows / B || n_batches > rows / B - first_batch)
        return fail(n, -1, "train_epoch: (first_batch + n_batches) * B must not exceed n (a remainder of less than B rows is not trained on)");
    if (aug) { const char* why = augment_refusal(aug, n->in_h, n->in_w); if (why) return fail(n, -1, std::string("train_epoch: ") + why); }
    if (n_batches == 0) return 0;
    Dev g(n->device);
    RTRY(ensure_epoch_bufs(n));
    if (mix_dev) RTRY(ensure_mix_bufs(n));
    n->walk_open = false;
    float* const xb = (float*)n->xb.p;
    int32_t* const yb = (int32_t*)n->yb.p;
    float* const el = (float*)n->eloss.p;
    float* const elr = (float*)n->elr.p;
    // the step on the net's own buffers -- mixed: its loss launch reads the two labels buffers and the weight scalar; scheduled: its update
    // reads the rate scalar -- so ONE graph serves every batch
    const StepKey key{xb, yb, mix_dev ? (const int32_t*)n->yb2.p : nullptr, mix_dev ? (const float*)n->emixw.p : nullptr, B, lr_dev ? 0.f : lr, lr_dev ? elr : nullptr, el};
    for (int64_t s = first_batch; s < first_batch + n_batches; ++s) {
        const rcn_hipx_mix_step* const rec = mix_dev ? mix_dev + (s - first_batch) : nullptr;
        RTRY(launch_gather(n, X, x_kind, x_scale, x_shift, labels, (long long)rows, perm ? perm + s * B : nullptr, (long long)s * B, B, aug, (unsigned long long)s * (unsigned long long)B, xb, yb,
                           rec, (int*)n->yb2.p));
        // the step's rate (and target weight) into the net's scalars, outside the graph: the eager step and every replay read them there
        // (an accumulating net: only the micro-step that applies the update reads a rate)
        const int micro = next_micro(n);
        if (lr_dev && (micro == kWholeStep || micro == kMicroLast)) XTRY(n, hipMemcpyAsync(elr, lr_dev + (s - first_batch), sizeof(float), hipMemcpyDeviceToDevice, n->stream));
        if (rec) XTRY(n, hipMemcpyAsync(n->emixw.p, &rec->weight, sizeof(float), hipMemcpyDeviceToDevice, n->stream));
        RTRY(training_step(n, key));
        if (loss_dev) XTRY(n, hipMemcpyAsync(loss_dev + (s - first_batch), el, sizeof(float), hipMemcpyDeviceToDevice, n->stream));
    }
    return 0;
}

int rcn_hipx_train_epoch_ex_dev(rcn_hipx_net* n, const void* X, int x_kind, float x_scale, float x_shift, const int32_t* labels, int64_t rows, const int32_t* perm,
                                int B, int64_t first_batch, int64_t n_batches, float lr, const float* lr_dev, const rcn_hipx_augment* aug, float* loss_dev) {
    return rcn_hipx_train_epoch_mix_dev(n, X, x_kind, x_scale, x_shift, labels, rows, perm, B, first_batch, n_batches, lr, lr_dev, aug, nullptr, loss_dev);
}

int rcn_hipx_train_epoch_dev(rcn_hipx_net* n, const void* X, int x_kind, float x_scale, float x_shift, const int32_t* labels, int64_t rows, const int32_t* perm,
                             int B, int64_t first_batch, int64_t n_batches, float lr, float* loss_dev) {
    return rcn_hipx_train_epoch_ex_dev(n, X, x_kind, x_scale, x_shift, labels, rows, perm, B, first_batch, n_batches, lr, nullptr, nullptr, loss_dev);
}

int rcn_hipx_gather_batch_dev(rcn_hipx_net* n, const void* X, int x_kind, float x_scale, float x_shift, const int32_t* labels, int64_t rows, const int32_t* idx, int64_t base,
                              int B, const rcn_hipx_augment* aug, uint64_t q0, float* x_out, int32_t* labels_out) {
    if (!n) return -1;
    if (!X || !x_out) return fail(n, -1, "gather_batch: X_dev and x_out_dev must not be NULL");
    if (!x_kind_ok(x_kind)) return fail(n, -1, "gather_batch: x_kind must be RCN_HIPX_X_F32 or RCN_HIPX_X_U8");
    RTRY(ensure_batch(n, B));
    if (rows < 1) return fail(n, -1, "gather_batch: n must be at least 1");
    if (!idx && (base < 0 || base > rows - B)) return fail(n, -1, "gather_batch: without idx_dev, rows base .. base + B - 1 must lie inside the set");
    if (aug) { const char* why = augment_refusal(aug, n->in_h, n->in_w); if (why) return fail(n, -1, std::string("gather_batch: ") + why); }
    Dev g(n->device);
    const bool with_labels = labels && labels_out;
    return launch_gather(n, X, x_kind, x_scale, x_shift, with_labels ? labels : nullptr, (long long)rows, idx, (long long)base, B, aug, (unsigned long long)q0, x_out,
                         with_labels ? labels_out : nullptr);
}

int rcn_hipx_gather_mix_dev(rcn_hipx_net* n, const void* X, int x_kind, float x_scale, float x_shift, const int32_t* labels, int64_t rows, const int32_t* idx, int64_t base,
                            int B, const rcn_hipx_augment* aug, uint64_t q0, const rcn_hipx_mix_step* mix_dev, float* x_out, int32_t* labels_out, int32_t* labels_b_out) {
    if (!n) return -1;
    if (!X || !x_out || !mix_dev) return fail(n, -1, "gather_mix: X_dev, mix_dev and x_out_dev must not be NULL");
    if (!x_kind_ok(x_kind)) return fail(n, -1, "gather_mix: x_kind must be RCN_HIPX_X_F32 or RCN_HIPX_X_U8");
    RTRY(ensure_batch(n, B));
    if (rows < 1) return fail(n, -1, "gather_mix: n must be at least 1");
    if (!idx && (base < 0 || base > rows - B)) return fail(n, -1, "gather_mix: without idx_dev, rows base .. base + B - 1 must lie inside the set");
    if (aug) { const char* why = augment_refusal(aug, n->in_h, n->in_w); if (why) return fail(n, -1, std::string("gather_mix: ") + why); }
    Dev g(n->device);
    return launch_gather(n, X, x_kind, x_scale, x_shift, labels, (long long)rows, idx, (long long)base, B, aug, (unsigned long long)q0, x_out, labels_out, mix_dev, labels_b_out);
}

int rcn_hipx_augment_draw(const rcn_hipx_augment* aug, uint64_t q, int* dy, int* dx, int* flip) {
    if (!aug || augment_refusal(aug, 0, 0)) return -1;
    const AugDraw d = augment_draw(AugSpec{aug->seed, aug->epoch, aug->pad, aug->hflip}, (unsigned long long)q);
    if (dy) *dy = d.dy;
    if (dx) *dx = d.dx;
    if (flip) *flip = d.flip;
    return 0;
}

int rcn_hipx_evaluate_dev(rcn_hipx_net* n, const void* X, int x_kind, float x_scale, float x_shift, const int32_t* labels, int64_t rows,
                          double* loss_sum, int64_t* correct, int32_t* pred) {
    return rcn_hipx_evaluate_ex_dev(n, X, x_kind, x_scale, x_shift, labels, rows, RCN_HIPX_WEIGHTS_LIVE, loss_sum, correct, pred);
}

int rcn_hipx_evaluate_ex_dev(rcn_hipx_net* n, const void* X, int x_kind, float x_scale, float x_shift, const int32_t* labels, int64_t rows, int weights,
                             double* loss_sum, int64_t* correct, int32_t* pred) {
    if (!n) return -1;
    return evaluate_rows(n, X, x_kind, x_scale, x_shift, labels, rows, weights, loss_sum, correct, pred, nullptr);
}

int rcn_hipx_evaluate_metrics_dev(rcn_hipx_net* n, const void* X, int x_kind, float x_scale, float x_shift, const int32_t* labels, int64_t rows, int weights,
                                  const rcn_hipx_eval_out* out) {
    if (!n) return -1;
    if (const char* why = metrics_refusal(out, n->classes, labels != nullptr)) return fail(n, -1, std::string("evaluate_metrics: ") + why);
    return evaluate_rows(n, X, x_kind, x_scale, x_shift, labels, rows, weights, out->loss_sum, out->correct, out->pred, out);
}

int rcn_hipx_label_rank(const float* row, int classes, int label, int* rank) {
    if (!row || !rank || classes < 1) return -1;
    *rank = label_rank(row, classes, label);
    return 0;
}

int rcn_hipx_graphs_instantiated(const rcn_hipx_net* n, int64_t* count) {
    if (!n || !count) return -1;
    *count = n->n_instantiated;
    return 0;
}

int rcn_hipx_gradients_dev(rcn_hipx_net* n, const float* x, const int32_t* labels, int B, float* grad, float* loss_dev) {
    if (!n || !x || !labels || !grad) return -1;
    RTRY(ensure_batch(n, B));
    Dev g(n->device);
    n->walk_open = false;
    XTRY(n, hipMemsetAsync(grad, 0, (size_t)n->n_pad * sizeof(float), n->stream));
    return step_core(n, x, labels, B, 0.f, grad, false, loss_dev);
}

int rcn_hipx_gradients_begin_dev(rcn_hipx_net* n, const float* x, const int32_t* labels, int B, float* grad, float* loss_dev, int64_t min_bucket_bytes, int* n_buckets) {
    if (!n || !x || !labels || !grad || !n_buckets || min_bucket_bytes < 0) return -1;
    RTRY(ensure_batch(n, B));
    Dev g(n->device);
    n->walk_open = false;
    XTRY(n, hipMemsetAsync(grad, 0, (size_t)n->n_pad * sizeof(float), n->stream));
    const int nb = grad_begin(n, x, labels, B, grad, loss_dev, (long long)min_bucket_bytes);
    if (nb < 0) return nb;
    *n_buckets = nb;
    n->walk_open = true;
    return 0;
}

int rcn_hipx_gradients_bucket_dev(rcn_hipx_net* n, int k, int64_t* off, int64_t* len) {
    if (!n) return -1;
    Dev g(n->device);
    long long o = 0, l = 0;
    RTRY(grad_bucket(n, k, &o, &l));
    if (n->bw.taken == (int)n->bw.lo.size()) n->walk_open = false;      // the last bucket: the walk is over
    if (off) *off = o;
    if (len) *len = l;
    return 0;
}

int rcn_hipx_step_flops(const rcn_hipx_net* n, int B, double* flops) {
    if (!n || !flops) return -1;
    double f = 0;
    for (size_t i = 0; i < n->L.size(); ++i) {
        const Layer& l = n->L[i];
        if (!l.row().matrix) continue;
        const double macs = (double)B * l.oH * l.oW * (double)l.K * l.Cout * 1.0;
        f += 2.0 * macs * (i == 0 ? 2.0 : 3.0);         // forward + wgrad (+ dgrad except for the first layer)
    }
    *flops = f;
    return 0;
}

int rcn_hipx_plan(int in_h, int in_w, int in_c, const rcn_hipx_layer* layers, int n_layers, int batch, int precision, int tiling, char* out, int cap) {
    if (!plan_args_ok(in_h, in_w, in_c, layers, n_layers, batch, precision, tiling, out, cap)) return -1;
    rcn_hipx_net net;                                   // (its options: as a net created now would have them; rcn_hipx_plan_net: an existing net's own)
    int st = make_dry_net(net, in_h, in_w, in_c, layers, n_layers, batch, precision, tiling);
    if (st == 0) {
        net.plan = step_header(net, batch);
        st = step_core(&net, nullptr, nullptr, batch, 0.f, nullptr, true, nullptr);
    }
    return emit(net, st, out, cap);
}

// The bucketed gradient step of a data-parallel rank, launch by launch and bucket by bucket (no GPU needed): forward + loss, then for every
// bucket the backward pass of its layers, the ONE reduction launch of their slabs, and the slice of the flat gradient that is final there.
int rcn_hipx_plan_buckets(int in_h, int in_w, int in_c, const rcn_hipx_layer* layers, int n_layers, int batch, int precision, int tiling, int64_t min_bucket_bytes,
                          char* out, int cap) {
    if (!plan_args_ok(in_h, in_w, in_c, layers, n_layers, batch, precision, tiling, out, cap) || min_bucket_bytes < 0) return -1;
    rcn_hipx_net net;
    int st = make_dry_net(net, in_h, in_w, in_c, layers, n_layers, batch, precision, tiling);
    if (st == 0) {
        net.plan = "gradients of one batch of " + std::to_string(batch) + " in buckets of at least " + std::to_string((long long)min_bucket_bytes) +
                   " bytes (data-parallel step: a bucket's all-reduce overlaps the backward pass below it):\n";
        const int nb = grad_begin(&net, nullptr, nullptr, batch, reinterpret_cast<float*>(sizeof(float)), nullptr, (long long)min_bucket_bytes);
        st = nb < 0 ? nb : 0;
        for (int k = 0; st == 0 && k < nb; ++k) st = grad_bucket(&net, k, nullptr, nullptr);
    }
    return emit(net, st, out, cap);
}

// the same walk for an EXISTING net, with that net's own precision, tiling, options and optimiser
int rcn_hipx_plan_net(const rcn_hipx_net* n, int batch, char* out, int cap) {
    if (!n || batch < 1 || batch > n->max_batch || !out || cap < 1) return -1;
    rcn_hipx_net net;
    make_dry_net(net, *n, batch);
    net.plan = step_header(net, batch);
    // (an accumulating net: the last micro-step of a cycle, the one that applies the update; rcn_hipx_plan_micro_net: the others)
    const int st = step_core(&net, nullptr, nullptr, batch, 0.f, nullptr, true, nullptr, nullptr, Pair{}, n->accum_k > 1 ? kMicroLast : kWholeStep);
    return emit(net, st, out, cap);
}

// One micro-step of an accumulating net, by kind: 0 the first of a cycle, 1 a middle one, 2 the last
int rcn_hipx_plan_micro_net(const rcn_hipx_net* n, int batch, int kind, char* out, int cap) {
    if (!n || batch < 1 || batch > n->max_batch || !out || cap < 1 || kind < 0 || kind > 2 || n->accum_k == 1) return -1;
    rcn_hipx_net net;
    make_dry_net(net, *n, batch);
    net.plan = step_header(net, batch);
    const int st = step_core(&net, nullptr, nullptr, batch, 0.f, nullptr, true, nullptr, nullptr, Pair{}, kind == 0 ? kMicroFirst : kind == 1 ? kMicroMiddle : kMicroLast);
    return emit(net, st, out, cap);
}

// One step of an epoch of an EXISTING net (rcn_hipx_train_epoch_mix_dev): what is launched around the captured graph -- the gather, the copy
// of a scheduled rate, the copy of a mixed step's target weight -- the graph's key, then the step's own plan (rcn_hipx_plan_net's walk; the _dlr update kernel for a scheduled rate).
int rcn_hipx_plan_epoch_mix_net(const rcn_hipx_net* n, int batch, int x_kind, int lr_from_device, const rcn_hipx_augment* aug, int mix, char* out, int cap) {
    if (!n || batch < 1 || batch > n->max_batch || !out || cap < 1) return -1;
    if (!x_kind_ok(x_kind) || (lr_from_device != 0 && lr_from_device != 1) || (mix != 0 && mix != 1)) return -1;
    if (aug) { const char* why = augment_refusal(aug, n->in_h, n->in_w); if (why) { std::snprintf(out, (size_t)cap, "%s", why); return -1; } }
    rcn_hipx_net net;
    make_dry_net(net, *n, batch);
    net.plan = "one step of an epoch over a resident " + std::string(x_kind == RCN_HIPX_X_U8 ? "uint8" : "fp32") + " set at batch " + std::to_string(batch) +
               ": the launches around the captured graph, its key, then the graph's own launches:\n";
    const float* const marker = reinterpret_cast<const float*>(sizeof(float));      // (dry run: no buffers; any non-null marks "the rate comes from the device")
    // (... and "a record" / "pair labels")
    const rcn_hipx_mix_step* const rec = mix ? reinterpret_cast<const rcn_hipx_mix_step*>(sizeof(float)) : nullptr;
    const Pair pair = mix ? Pair{reinterpret_cast<const int32_t*>(sizeof(float)), marker} : Pair{};
    int st = launch_gather(&net, nullptr, x_kind, 1.f, 0.f, nullptr, 1, nullptr, 0, batch, aug, 0, nullptr, nullptr, rec, nullptr);
    if (st == 0) {
        if (lr_from_device) (void)dry_note(&net, "  lr: 4-byte device copy of lr_dev[i] into the net's rate scalar (hipMemcpyAsync, outside the graph)");
        if (mix) (void)dry_note(&net, "  weight: 4-byte device copy of mix_dev[i].weight into the net's target-weight scalar (hipMemcpyAsync, outside the graph)");
        if (n->accum_k > 1)
            // an accumulating net keeps a graph per kind of micro-step; only the last kind applies a rate
            (void)dry_note(&net, "  graph: one graph per kind of micro-step (first%s, last) and B; the last kind %s%s -- below: the last kind", n->accum_k > 2 ? ", middle" : "",
                           lr_from_device ? "with lr from device" : "per (B, lr)", mix ? ", pair labels" : "");
        else if (mix) (void)dry_note(&net, lr_from_device ? "  graph: one graph per B, lr from device, pair labels" : "  graph: one graph per (B, lr), pair labels");
        else (void)dry_note(&net, lr_from_device ? "  graph: one graph per B, lr from device" : "  graph: one graph per (B, lr)");
        net.plan += step_header(net, batch);
        st = step_core(&net, nullptr, nullptr, batch, 0.f, nullptr, true, nullptr, lr_from_device ? marker : nullptr, pair, n->accum_k > 1 ? kMicroLast : kWholeStep);
    }
    return emit(net, st, out, cap);
}

int rcn_hipx_plan_epoch_net(const rcn_hipx_net* n, int batch, int x_kind, int lr_from_device, const rcn_hipx_augment* aug, char* out, int cap) {
    return rcn_hipx_plan_epoch_mix_net(n, batch, x_kind, lr_from_device, aug, 0, out, cap);
}

// rcn_hipx_plan's dry walk for ONE evaluation chunk: the forward pass over all layers and the evaluation kernel.  A net that
// rcn_hipx_set_precision would refuse (RCN_HIPX_BF16_STORED on layers the bf16-tensor kernels do not cover) is refused here with the same text.
int rcn_hipx_plan_eval(int in_h, int in_w, int in_c, const rcn_hipx_layer* layers, int n_layers, int batch, int precision, int tiling, char* out, int cap) {
    if (!plan_args_ok(in_h, in_w, in_c, layers, n_layers, batch, precision, tiling, out, cap)) return -1;
    rcn_hipx_net net;
    int st = make_dry_net(net, in_h, in_w, in_c, layers, n_layers, batch, precision, tiling);
    if (st == 0 && net.store16) {
        std::string why;
        st = store16_covered(net, &why);
        if (st != 0) net.err = why;
    }
    if (st == 0) st = plan_eval_walk(net, batch);
    return emit(net, st, out, cap);
}

// the same walk for an EXISTING net, with that net's own precision, tiling and options
int rcn_hipx_plan_eval_net(const rcn_hipx_net* n, int batch, char* out, int cap) {
    if (!n || batch < 1 || batch > n->max_batch || !out || cap < 1) return -1;
    rcn_hipx_net net;
    make_dry_net(net, *n, batch);
    const int st = plan_eval_walk(net, batch);
    return emit(net, st, out, cap);
}

// ... and for one chunk of a metrics call that asks for n_topk counts and (flags) the confusion matrix, the per-row results and the logits
int rcn_hipx_plan_eval_metrics_net(const rcn_hipx_net* n, int batch, int n_topk, int confusion, int per_row, int logits, char* out, int cap) {
    if (!n || batch < 1 || batch > n->max_batch || n_topk < 0 || n_topk > RCN_HIPX_EVAL_MAX_TOPK || !out || cap < 1) return -1;
    rcn_hipx_net net;
    make_dry_net(net, *n, batch);
    // the dry walk only asks which outputs are wanted: no pointer of `ask` is read through
    static int64_t marker64;
    static float marker32;
    static int32_t marker_i;
    rcn_hipx_eval_out ask{};
    ask.n_topk = n_topk;
    ask.topk_correct = n_topk > 0 ? &marker64 : nullptr;
    ask.confusion = confusion ? &marker64 : nullptr;
    ask.loss_each = per_row ? &marker32 : nullptr;
    ask.rank = per_row ? &marker_i : nullptr;
    ask.logits = logits ? &marker32 : nullptr;
    const int st = plan_eval_walk(net, batch, &ask);
    return emit(net, st, out, cap);
}

}  // extern "C"

#include "rcn_hipx_api_update.ipp"
#include "rcn_hipx_api_dropout.ipp"
#include "rcn_hipx_api_state.ipp"
#include "rcn_hipx_api_bn.ipp"
