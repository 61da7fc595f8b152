// rcn_hip_api.hip -- the C ABI of include/rcn_hip.h on top of the gfx950 kernels.
// Host logic here mirrors the bookkeeping of RCN::{new, load_weights_and_bias, train_batch, classify}
// (rcn/src/rcn.rs); all arithmetic on sample data happens in the HIP kernels -- there is no CPU fallback.
#include "../../include/rcn_hip.h"

#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <functional>
#include <map>
#include <mutex>
#include <new>
#include <random>
#include <string>
#include <tuple>
#include <vector>

#include "common.hpp"
#include "dense.hpp"
#include "dense_pipe.hpp"
#include "dense_wide.hpp"
#include "dense_p2.hpp"
#include "features.hpp"
#include "ops.hpp"
#include "dp_rccl.hpp"
#include "serve.hpp"
#include "dp_p2p.hpp"
#include "dense_p2_dp.hpp"
#include "dense_xcd.hpp"
#include <atomic>
#include <chrono>

using namespace rcn;

namespace {

struct DevBuf {
    void* p = nullptr;
    size_t cap = 0;
    hipError_t ensure(size_t bytes) {
        if (bytes <= cap) return hipSuccess;
        if (p) { (void)hipFree(p); p = nullptr; cap = 0; }
        size_t want = bytes < 4096 ? 4096 : bytes;
        hipError_t e = hipMalloc(&p, want);
        if (e == hipSuccess) cap = want;
        return e;
    }
    void release() { if (p) (void)hipFree(p); p = nullptr; cap = 0; }
};

struct EpochKey {
    const void* X; const void* Y; const void* perm; size_t B; size_t nb; double eta; const void* loss; size_t j0 = 0;
    bool operator<(const EpochKey& o) const {
        return std::tie(X, Y, perm, B, nb, eta, loss, j0) < std::tie(o.X, o.Y, o.perm, o.B, o.nb, o.eta, o.loss, o.j0);
    }
};

}  // namespace

// Per-context options (rcn_hip_set_option / rcn_hip_get_option).  The environment variable of the same meaning only SEEDS the default
// when the context is created; two contexts of one process can differ, and nothing reads the environment afterwards.
struct CtxOptions {
    long long xcd = 1;                  // "xcd"               RCN_HIP_XCD            0: dense path 0 (auto) never selects the resident one-XCD kernel
    long long xcd_select = 0;           // "xcd_select"        RCN_HIP_XCD_SELECT     TEST-ONLY: which blocks are the workers -- 0..7: blockIdx.x % 8 == this; 8..15: the
                                        //                                            blocks that landed on PHYSICAL XCD this - 8 (ranks sharing one device)
    long long xcd_gather = 0;           // "xcd_gather"        RCN_HIP_XCD_GATHER     1: rows fetched by the resident kernel itself (B = 256; measured slower, still)
    long long xcd_timeout_ticks = 20000000;   // "xcd_timeout_ticks"            bound of every wait inside the resident kernel, 100 MHz ticks (0.2 s)
    long long xcd_exact_lds = 0;        // "xcd_exact_lds"                            1: the resident kernel asks for exactly the LDS it uses (two workers may share a CU:
                                        //                                            what lets two contexts' kernels be resident on ONE device); 0: at least half a CU's
    long long xcd_dp_phase = 0;         // "xcd_dp_phase"                             DIAGNOSTIC: data-parallel launches at a shard of 256 carry per-worker phase clocks
    long long xcd_fault_launch = 0;     // "xcd_fault_launch"                         TEST HOOK: the n-th resident launch of the context (1-based) loses a worker
    long long xcd_fault_mode = 0;       // "xcd_fault_mode"                           TEST HOOK: how -- 0 worker 1 never becomes resident, 1 it reaches the closing round late
    long long xcd_auto_fallback = 1;    // "xcd_auto_fallback"                        1: an expired wait of the single-GPU resident kernel re-runs the segment on the two-kernel pipeline
    long long xcd_replay_caller_rows = 0;   // "xcd_replay_caller_rows"               1: that re-run may also read index rows the CALLER wrote (taken as unchanged since the call); 0: only
                                        //                                            stored-order calls and rows the library shuffled / uploaded itself are re-run, anything else is an error
    long long dp_p2p = 1;               // "dp_p2p"            RCN_HIP_DP_P2P         0: no peer exchange (ncclAllReduce), 1: when world > 1, 2: also at world 1
    long long dp_fused = 1;             // "dp_fused"          RCN_HIP_DP_FUSED       0: the exchange never runs inside a step kernel
    long long dp_timeout_ticks = 100000000;   // "dp_timeout_ticks" RCN_HIP_DP_TIMEOUT_TICKS  bound of a peer wait, 100 MHz ticks (1 s)
    long long dp_cached_buf = 0;        // "dp_cached_buf"     RCN_HIP_DP_CACHED_BUF  1: exported buffers in ordinary (cached) device memory (A/B measurements)
    long long dp_graph = 1;             // "dp_graph"          RCN_HIP_DP_GRAPH       0: the three-kernel data-parallel step is enqueued eagerly
    long long feat_waves = 1;           // "feat_waves"        RCN_HIP_FEAT_WAVES     2: two waves per picture in k_features_cpcp (measured neutral)
    long long no_fragimg = 0;           // "no_fragimg"        RCN_HIP_NO_FRAGIMG     1: k_p2_b gathers its tail parameters itself
    long long exact_div_only = 0;       // "exact_div_only"    RCN_HIP_EXACT_DIV_ONLY 1: the f32 standardisation always divides
    long long pack_segment_bytes = (long long)64 << 20;   // "pack_segment_bytes" RCN_HIP_PACK_SEGMENT_BYTES  one half of the epoch image
    long long pack_form = 1;            // "pack_form"         RCN_HIP_PACK_FORM      1: the epoch image is gathered by k_pack_rows (whole rows, no load chains); 0: by k_pack_epoch
};

namespace {
struct OptDesc { const char* name; const char* env; long long CtxOptions::*field; long long lo, hi; };
const OptDesc kOptTable[] = {
    {"xcd", "RCN_HIP_XCD", &CtxOptions::xcd, 0, 1},
    {"xcd_select", "RCN_HIP_XCD_SELECT", &CtxOptions::xcd_select, 0, 15},
    {"xcd_gather", "RCN_HIP_XCD_GATHER", &CtxOptions::xcd_gather, 0, 1},
    {"xcd_timeout_ticks", "RCN_HIP_XCD_TIMEOUT_TICKS", &CtxOptions::xcd_timeout_ticks, 1, 1LL << 40},
    {"xcd_exact_lds", "RCN_HIP_XCD_EXACT_LDS", &CtxOptions::xcd_exact_lds, 0, 1},
    {"xcd_auto_fallback", "RCN_HIP_XCD_AUTO_FALLBACK", &CtxOptions::xcd_auto_fallback, 0, 1},
    {"xcd_replay_caller_rows", "RCN_HIP_XCD_REPLAY_CALLER_ROWS", &CtxOptions::xcd_replay_caller_rows, 0, 1},
    {"xcd_fault_launch", "RCN_HIP_XCD_FAULT_LAUNCH", &CtxOptions::xcd_fault_launch, 0, 0x7fffffff},
    {"xcd_fault_mode", "RCN_HIP_XCD_FAULT_MODE", &CtxOptions::xcd_fault_mode, 0, 1},
    {"xcd_dp_phase", "RCN_HIP_XCD_DP_PHASE", &CtxOptions::xcd_dp_phase, 0, 1},
    {"dp_p2p", "RCN_HIP_DP_P2P", &CtxOptions::dp_p2p, 0, 2},
    {"dp_fused", "RCN_HIP_DP_FUSED", &CtxOptions::dp_fused, 0, 1},
    {"dp_timeout_ticks", "RCN_HIP_DP_TIMEOUT_TICKS", &CtxOptions::dp_timeout_ticks, 1, 1LL << 40},
    {"dp_cached_buf", "RCN_HIP_DP_CACHED_BUF", &CtxOptions::dp_cached_buf, 0, 1},
    {"dp_graph", "RCN_HIP_DP_GRAPH", &CtxOptions::dp_graph, 0, 1},
    {"feat_waves", "RCN_HIP_FEAT_WAVES", &CtxOptions::feat_waves, 1, 2},
    {"no_fragimg", "RCN_HIP_NO_FRAGIMG", &CtxOptions::no_fragimg, 0, 1},
    {"exact_div_only", "RCN_HIP_EXACT_DIV_ONLY", &CtxOptions::exact_div_only, 0, 1},
    {"pack_segment_bytes", "RCN_HIP_PACK_SEGMENT_BYTES", &CtxOptions::pack_segment_bytes, 1, 1LL << 40},
    {"pack_form", "RCN_HIP_PACK_FORM", &CtxOptions::pack_form, 0, 1},
};
}  // namespace

struct rcn_hip_ctx {
    int device = 0;
    int dtype = RCN_HIP_F32;
    CtxOptions opt;
    std::string dp_fault;                   // RCN_HIP_DP_FAULT as it was when the context was created (fault injection for the admission tests)
    hipStream_t stream = nullptr;
    bool own_stream = false;
    FeatDesc fd{};
    NetDesc nd{};
    int n_conv = 0;
    bool params_set = false;
    std::string dense_err;                  // non-empty: every dense call panics in the reference (see rcn_hip_create)
    double mean = 1.0, sd = 1.0;            // scale_set initial value (1,1): rcn.rs:71
    int feat_kernel = 0;                    // 0 auto, 1 always the generic k_features (tests compare the two)
    float fd_mean = 0.f, fd_sd = 0.f, fd_rcp = 0.f;   // last (mean, sd) checked by standardise_fast_is_exact; fd_rcp = 0: divide
    bool fd_checked = false;
    int dense_path = 0;                     // 0 auto, 1 sample-tile kernels (dense.hpp), 2 feature-sliced pipeline (dense_pipe.hpp)
    DevBuf slab, xpack, ypack, p2buf;
    DevBuf fragimg;                         // tail parameters as k_p2_b's operand fragments (dense.hpp: p2_frag_scatter), f32 pipeline only
    bool frag_on = false;                   // set while enqueue_pipe_steps<float> runs: its k_p2_a / k_p2_b launches use the image
    size_t packed_B = 0, packed_nb = 0;     // what the epoch image currently holds (k_pack_epoch)
    size_t epoch_B = 0, epoch_nb = 0, epoch_seg = 0;   // rcn_hip_epoch_begin*_dev: the image holds batches 0..epoch_nb of a begun epoch
                                                       // (epoch_nb = 0: none; any other call that re-packs the image ends it)
    void* pin_host = nullptr;               // small pinned, device-mapped staging block for the serving path (classify)
    void* pin_dev = nullptr;
    DevBuf params, acts, deltas, loss_part, grad, xstage, ystage, ostage, scratch0, scratch1, scratch2, redpart, misc;
    std::map<EpochKey, hipGraphExec_t> graphs, dp_graphs, img_graphs, step_graphs;
    ncclComm_t comm = nullptr;              // data-parallel group (rcn_hip_dp_init); one rank per context
    int dp_rank = 0, dp_world = 1;
    struct P2P {                            // peer-read all-reduce over xGMI (dp_p2p.hpp)
        bool exported = false, attached = false, on = false;
        bool fused = false;                 // the exchange may run inside the gradient kernel (passed its own known-answer vote)
        bool push = false;                  // the pushed reduce-scatter + all-gather of the resident kernel passed its vote (dp_push.hpp)
        size_t push_off = 0;                // byte offset of its region in every rank's exported buffer
        void* local_buf = nullptr;          // [2][stride] values + [2][stride] tagged words + the pushed exchange's rows, uncached device memory
        size_t local_bytes = 0, flags_cap = 0;
        bool local_uncached = false;
        unsigned* local_flags = nullptr;    // [kP2PMaxWorld], uncached device memory
        void* peer_buf[rcn::kP2PMaxWorld] = {};
        unsigned* peer_flags[rcn::kP2PMaxWorld] = {};
        size_t stride = 0;                  // values per slot (>= P+1, multiple of 4)
        unsigned seq = 0;                   // step sequence number, identical on every rank
        unsigned* err_dev = nullptr;        // sticky: 1 + rank that timed out; err_dev[16] = sequence base read by replayed graphs
        unsigned* err_host = nullptr;       // pinned copy, refreshed after every epoch call
        DevBuf raw, mism;
    } p2p;
    DevBuf xcdbuf;                          // one-XCD resident epoch kernel (dense_xcd.hpp): slab, deltas, fragment image, flags
    size_t xcd_B = 0;
    unsigned xcd_tag = 0;                   // last step tag handed out; monotonic for the life of the buffer
    unsigned* xerr_host = nullptr;          // its sticky error word: pinned host memory the kernel writes straight into (no copy-back in the stream)
    unsigned* xerr_dev = nullptr;
    struct { const float* X = nullptr; const float* Y = nullptr; const int32_t* perm = nullptr; size_t B = 0, nb = 0; } xg;   // the last call the resident
                                            // kernel ran in its gather form (rcn_hip_time_kernels_dev times that form over the same rows)
    bool xcd_dp_used = false;               // the resident kernel ran data-parallel steps since dp_init: dp_finalize clears its timeout word
    bool xcd_stepped_down = false;          // a wait of the resident kernel expired and the library stepped this context down to the two-kernel pipeline
    unsigned xcd_launch_id = 0;             // id of the newest resident launch enqueued (the kernel reports the newest COMPLETE one in xerr_host[1])
    unsigned long long xcd_launches = 0;    // resident launches of this context so far (option "xcd_fault_launch" counts them)
    int fallbacks_taken = 0;                // rcn_hip_fallbacks_taken
    bool replaying = false;                 // the redo log is being replayed: nothing is logged
    // Redo log of the training calls whose resident launches have not been seen complete yet (dense_xcd.hpp: parameters are written only
    // by a launch ALL of whose workers finished, and a launch that finds the error word set leaves at once -- so after a failure the
    // parameters are the state after launch xerr_host[1], and everything enqueued behind it can be re-run on the two-kernel pipeline).
    struct PermSource {                      // how a call's index rows came to be: a device shuffle (re-drawn from its seed) or a host upload (kept)
        int kind = 0;                        // 0 none (caller's buffer, taken as unchanged), 1 rcn_hip_shuffle_dev, 2 upload
        int32_t* buf = nullptr; size_t n = 0, passes = 0; uint64_t seed = 0;
        std::vector<int32_t> host;
    };
    struct XcdLaunchRec { unsigned id; size_t k0, n; };
    struct BeginRec {                        // the arguments of the newest rcn_hip_epoch_begin*_dev (the epoch image can be laid out again from them)
        const void* X = nullptr; const void* Y = nullptr; const int32_t* perm = nullptr; size_t B = 0, nb = 0; bool from_images = false; bool valid = false;
        PermSource src;
    };
    struct RedoRec {
        int kind = 0;                        // 0 train_epoch (X, Y, perm), 1 epoch_steps on the image of `begin`
        const void* X = nullptr; const void* Y = nullptr; const int32_t* perm = nullptr;
        size_t B = 0, nb = 0, j0 = 0; double eta = 0; void* loss_dev = nullptr; bool from_images = false;
        PermSource src;
        BeginRec begin;
        bool caller_rows = false;            // the call's index rows were written by the caller (not by rcn_hip_shuffle_dev / an upload of the library)
        std::vector<XcdLaunchRec> launches;
    };
    std::vector<RedoRec> redo;
    std::vector<PermSource> perm_sources;    // newest source per index buffer
    BeginRec last_begin;
    unsigned* xerrd = nullptr;               // device copy of the resident kernel's sticky error word (outlives every workspace reset)
    unsigned xrec[16] = {};                  // the newest time-out record (dense_xcd.hpp: xcd_raise; [kXcdRecWords] = the error code), kept past a heal
    bool xrec_valid = false;
    std::string xlast;                       // ... and its text with the workspace's tables (rcn_hip_last_timeout_text)
    int xcd_probe = 0;                      // 0 not probed, 1 the blocks with equal b % 8 share one XCD and the eight classes sit on eight XCDs, -1 not so
    struct ResidentSet {                     // rcn_hip_load_data: one of RCN::train's two data sets, kept in HBM (rcn.rs:134-137)
        DevBuf imgs, X, Y, perm, loss;
        size_t n = 0;
    } sets[2];
    std::map<const void*, size_t> lds_attr;   // kernels whose dynamic-LDS limit was already raised
    std::string err;
    size_t esz() const { return dtype == RCN_HIP_F64 ? 8 : 4; }
};

namespace {

int fail(rcn_hip_ctx* c, int code, const std::string& msg) {
    if (c) c->err = msg;
    return code;
}

#define HIP_TRY(ctx, expr)                                                                                   \
    do {                                                                                                     \
        hipError_t e_ = (expr);                                                                              \
        if (e_ != hipSuccess)                                                                                \
            return fail(ctx, e_ == hipErrorOutOfMemory ? RCN_HIP_ERR_OOM : RCN_HIP_ERR_HIP,                  \
                        std::string(#expr) + ": " + hipGetErrorString(e_));                                  \
    } while (0)

#define RCN_TRY(expr)                      \
    do {                                   \
        int s_ = (expr);                   \
        if (s_ != RCN_HIP_OK) return s_;   \
    } while (0)

struct DevGuard {
    int prev = -1;
    explicit DevGuard(int dev) { (void)hipGetDevice(&prev); if (prev != dev) (void)hipSetDevice(dev); else prev = -1; }
    ~DevGuard() { if (prev >= 0) (void)hipSetDevice(prev); }
};

#include "rcn_hip_api_shapes.ipp"
#include "rcn_hip_api_dense_launch.ipp"
#include "rcn_hip_api_xcd.ipp"
#include "rcn_hip_api_p2p.ipp"
// =====================================================================================================================
extern "C" {

int rcn_hip_abi_version(void) { return RCN_HIP_ABI_VERSION; }

const char* rcn_hip_status_string(int s) {
    switch (s) {
    case RCN_HIP_OK: return "ok";
    case RCN_HIP_ERR_INVALID_ARG: return "invalid argument";
    case RCN_HIP_ERR_SHAPE: return "shape error (the reference panics here)";
    case RCN_HIP_ERR_UNSUPPORTED: return "unsupported (not implemented in the reference, or over a size limit)";
    case RCN_HIP_ERR_HIP: return "HIP runtime error";
    case RCN_HIP_ERR_NO_DEVICE: return "no usable HIP device";
    case RCN_HIP_ERR_STATE: return "call-order error";
    case RCN_HIP_ERR_OOM: return "out of device memory";
    default: return "unknown status";
    }
}

int rcn_hip_create(const rcn_hip_cfg* cfg, rcn_hip_ctx** out) {
    if (!cfg || !out) return RCN_HIP_ERR_INVALID_ARG;
    *out = nullptr;
    if (cfg->struct_size != sizeof(rcn_hip_cfg)) return RCN_HIP_ERR_INVALID_ARG;
    if (cfg->dtype != RCN_HIP_F32 && cfg->dtype != RCN_HIP_F64) return RCN_HIP_ERR_INVALID_ARG;
    if (cfg->n_convpool < 0 || cfg->n_convpool > kMaxConvPool || (cfg->n_convpool > 0 && !cfg->convpool)) return RCN_HIP_ERR_INVALID_ARG;
    if (cfg->n_hidden < 1 || cfg->n_hidden + 1 > kMaxLayers || !cfg->hidden) return RCN_HIP_ERR_INVALID_ARG;   // rcn.rs:444 indexes feedforward_cfg[0]
    if (cfg->classes < 1 || cfg->in_h < 1 || cfg->in_w < 1) return RCN_HIP_ERR_INVALID_ARG;
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0 || cfg->device < 0 || cfg->device >= ndev) return RCN_HIP_ERR_NO_DEVICE;

    rcn_hip_ctx* c = new (std::nothrow) rcn_hip_ctx();
    if (!c) return RCN_HIP_ERR_OOM;
    *out = c;                                   // handed back even on failure so the caller can read last_error
    c->device = cfg->device;
    c->dtype = cfg->dtype;
    if (const char* e = std::getenv("RCN_HIP_DP_FAULT")) c->dp_fault = e;
    for (const OptDesc& od : kOptTable) {             // the environment seeds the defaults, once, here
        const char* e = std::getenv(od.env);
        if (!e || !*e) continue;
        const long long v = std::atoll(e);
        if (v >= od.lo && v <= od.hi) c->opt.*(od.field) = v;
    }
    RCN_TRY(build_feat_desc(c, cfg));
    // RCN::new itself never fails; a stack whose dense part cannot run in the reference is remembered and
    // reported by the dense entry points (the reference panics inside train, not inside new).
    const long fan = first_layer_fan_in(cfg, c->fd.F);
    if (c->fd.F <= 0)
        c->dense_err = "the conv/pool stack yields an empty feature vector (no Convolve2D layer)";
    else if (fan != c->fd.F)
        c->dense_err = "first-layer fan-in 4^c/2^p*l (rcn.rs:443) = " + std::to_string(fan) + " differs from the flattened feature length " +
                       std::to_string(c->fd.F) + ": the reference panics in gemv (rcn.rs:287)";
    if (c->fd.F <= 0) c->fd.F = 0;
    {
        const int savedF = c->fd.F;
        if (savedF == 0) c->fd.F = 1;           // keep the dense bookkeeping well-formed; dense calls are refused anyway
        const int st = build_net_desc(c, cfg);
        c->fd.F = savedF;
        if (st != RCN_HIP_OK) return st;
    }
    DevGuard g(c->device);
    if (cfg->stream) { c->stream = (hipStream_t)cfg->stream; c->own_stream = false; }
    else { HIP_TRY(c, hipStreamCreateWithFlags(&c->stream, hipStreamNonBlocking)); c->own_stream = true; }
    HIP_TRY(c, c->params.ensure((size_t)c->nd.P * c->esz()));
    HIP_TRY(c, hipMemsetAsync(c->params.p, 0, (size_t)c->nd.P * c->esz(), c->stream));
    // (layer stacks whose tile image exceeds LDS run layer by layer on global activations: dense_wide.hpp)
    return RCN_HIP_OK;            // (feature maps that do not fit LDS are staged in global memory: k_features' `spill`)
}

void rcn_hip_destroy(rcn_hip_ctx* c) {
    if (!c) return;
    {
        DevGuard g(c->device);
        if (c->stream) (void)hipStreamSynchronize(c->stream);
        drop_graphs(c);
        if (c->comm) { (void)rcn::Rccl::get().CommDestroy(c->comm); c->comm = nullptr; }
        p2p_release(c);
        for (DevBuf* b : {&c->slab, &c->xpack, &c->ypack, &c->p2buf, &c->params, &c->acts, &c->deltas, &c->loss_part, &c->grad, &c->xstage, &c->ystage, &c->ostage, &c->scratch0,
                          &c->scratch1, &c->scratch2, &c->redpart, &c->misc})
            b->release();
        c->xcdbuf.release();
        if (c->xerr_host) (void)hipHostFree(c->xerr_host);
        if (c->xerrd) (void)hipFree(c->xerrd);
        for (auto& rs : c->sets) { rs.imgs.release(); rs.X.release(); rs.Y.release(); rs.perm.release(); rs.loss.release(); }
        if (c->pin_host) (void)hipHostFree(c->pin_host);
        if (c->own_stream && c->stream) (void)hipStreamDestroy(c->stream);
    }
    delete c;
}

const char* rcn_hip_last_error(const rcn_hip_ctx* c) { return c ? c->err.c_str() : "null context"; }

int rcn_hip_set_stream(rcn_hip_ctx* c, void* s) {
    RCN_TRY(check_ctx(c));
    DevGuard g(c->device);
    drop_graphs(c);
    if (c->own_stream && c->stream) { (void)hipStreamSynchronize(c->stream); (void)hipStreamDestroy(c->stream); }
    if (s) { c->stream = (hipStream_t)s; c->own_stream = false; }
    else { HIP_TRY(c, hipStreamCreateWithFlags(&c->stream, hipStreamNonBlocking)); c->own_stream = true; }
    return RCN_HIP_OK;
}

int rcn_hip_set_feature_kernel(rcn_hip_ctx* c, int mode) {
    RCN_TRY(check_ctx(c));
    if (mode < 0 || mode > 1) return fail(c, RCN_HIP_ERR_INVALID_ARG, "set_feature_kernel: mode must be 0 or 1");
    c->feat_kernel = mode;
    return RCN_HIP_OK;
}

int rcn_hip_set_dense_path(rcn_hip_ctx* c, int mode) {
    RCN_TRY(check_ctx(c));
    if (mode < 0 || mode > 5)
        return fail(c, RCN_HIP_ERR_INVALID_ARG, "set_dense_path: mode must be 0 (auto), 1 (sample-tile), 2 (feature-sliced, two kernels per step), 5 (feature-sliced, resident "
                                                "one-XCD kernel)");
    if (mode == 3 || mode == 4) return fail(c, RCN_HIP_ERR_UNSUPPORTED, "set_dense_path: modes 3 and 4 (one resident kernel per epoch segment, one launch per step) were removed");
    if (mode >= 2 && !pipe_supported(c->nd)) return fail(c, RCN_HIP_ERR_UNSUPPORTED, "feature-sliced path needs >= 2 dense layers whose tail fits LDS");
    DevGuard g(c->device);
    if (mode == 5) {
        if (!xcd_supported(c->nd, 32, c->esz()))
            return fail(c, RCN_HIP_ERR_UNSUPPORTED, "set_dense_path(5): the resident one-XCD kernel covers one hidden layer <= 32 (or two: <= 32, <= 16), classes <= 16, "
                                                      "at most 29 feature-slice pairs, batches of 1..256");
        RCN_TRY(xcd_probe(c));
        if (c->xcd_probe != 1)
            return fail(c, RCN_HIP_ERR_UNSUPPORTED, "set_dense_path(5): on this device the blocks with blockIdx.x % 8 == 0 do not share one XCD; the resident kernel "
                                                      "cannot be used");
    }
    drop_graphs(c);
    if (mode != 0 && mode != 5 && c->xerr_host && c->xerr_host[0] != 0 && !c->xcd_dp_used && !c->opt.xcd_auto_fallback) {
        // the recovery the error message names: leaving the resident kernel clears its sticky word (what it had not applied stays lost)
        HIP_TRY(c, hipStreamSynchronize(c->stream));
        RCN_TRY(xcd_clear_error(c));
        c->redo.clear();
    }
    if (mode == 5) c->xcd_stepped_down = false;
    c->dense_path = mode;
    return RCN_HIP_OK;
}

int rcn_hip_set_option(rcn_hip_ctx* c, const char* name, int64_t value) {
    RCN_TRY(check_ctx(c));
    if (!name) return fail(c, RCN_HIP_ERR_INVALID_ARG, "set_option: NULL name");
    for (const OptDesc& od : kOptTable)
        if (std::strcmp(od.name, name) == 0) {
            if (value < od.lo || value > od.hi)
                return fail(c, RCN_HIP_ERR_INVALID_ARG, std::string("set_option: ") + name + " must be in " + std::to_string(od.lo) + ".." + std::to_string(od.hi));
            if (c->opt.*(od.field) == (long long)value) return RCN_HIP_OK;
            DevGuard g(c->device);
            drop_graphs(c);                        // captured graphs bake in launch shapes, time-outs and the image's segment length
            if (od.field == &CtxOptions::pack_segment_bytes) c->epoch_nb = 0;
            c->opt.*(od.field) = (long long)value;
            return RCN_HIP_OK;
        }
    return fail(c, RCN_HIP_ERR_INVALID_ARG, std::string("set_option: unknown option '") + name + "'");
}

int rcn_hip_get_option(const rcn_hip_ctx* c, const char* name, int64_t* value) {
    if (!c || !name || !value) return RCN_HIP_ERR_INVALID_ARG;
    for (const OptDesc& od : kOptTable)
        if (std::strcmp(od.name, name) == 0) { *value = (int64_t)(c->opt.*(od.field)); return RCN_HIP_OK; }
    return RCN_HIP_ERR_INVALID_ARG;
}

int rcn_hip_fallbacks_taken(const rcn_hip_ctx* c) { return c ? c->fallbacks_taken : 0; }

int rcn_hip_synchronize(rcn_hip_ctx* c) {
    RCN_TRY(check_ctx(c));
    DevGuard g(c->device);
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    return sticky_errors(c);
}

int rcn_hip_feature_len(const rcn_hip_ctx* c, int64_t* out) {
    if (!c || !out) return RCN_HIP_ERR_INVALID_ARG;
    *out = c->fd.F;
    return RCN_HIP_OK;
}
int rcn_hip_num_layers(const rcn_hip_ctx* c) { return c ? c->nd.L : RCN_HIP_ERR_INVALID_ARG; }
int rcn_hip_layer_dims(const rcn_hip_ctx* c, int layer, int32_t* rows, int32_t* cols) {
    if (!c || !rows || !cols || layer < 0 || layer >= c->nd.L) return RCN_HIP_ERR_INVALID_ARG;
    *rows = c->nd.dims[layer + 1]; *cols = c->nd.dims[layer];
    return RCN_HIP_OK;
}
int rcn_hip_param_count(const rcn_hip_ctx* c, int64_t* out) {
    if (!c || !out) return RCN_HIP_ERR_INVALID_ARG;
    *out = c->nd.P;
    return RCN_HIP_OK;
}

#include "rcn_hip_api_params.ipp"
#include "rcn_hip_api_operators.ipp"
#include "rcn_hip_api_features.ipp"
#include "rcn_hip_api_dense.ipp"
#include "rcn_hip_api_dp.ipp"
#include "rcn_hip_api_sets.ipp"
}  // extern "C"
