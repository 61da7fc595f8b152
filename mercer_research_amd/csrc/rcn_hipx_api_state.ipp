// rcn_hipx_api_state.ipp -- part of rcn_hipx_api.hip (one translation unit): the whole training state of a net written down and picked up
// again (convnet_state.hpp).  The layout of a body (rcn_hipx_state_layout, pure host code), the one pack launch (rcn_hipx_snapshot_dev),
// the validated restore through the setters and the one unpack launch (rcn_hipx_restore_dev), and the accumulator's setter.

namespace {

static_assert(sizeof(rcn_hipx_state_desc) == 688, "rcn_hipx_state_desc is 688 bytes (mercer_research_amd/convnet.py: StateDesc)");
static_assert(sizeof(AdamTick) == kStateTickBytes && sizeof(long long) == kStateDropBytes && sizeof(unsigned long long) + 2 * sizeof(float) == kStateClipBytes,
              "the scalars block holds raw copies of the three buffers");
constexpr int kStateAllSections = (1 << kStateSections) - 1;

long long round256(long long bytes) { return (bytes + 255) / 256 * 256; }
// a layer's `out` as its description gave it, up to what create ignores: 0 for a layer without parameters (the two pools), the distance to
// the skip's source for RCN_HIPX_BN_ADD_RELU, the output width otherwise
int desc_out(const rcn_hipx_net& n, size_t i) {
    const Layer& l = n.L[i];
    return !l.row().params ? 0 : l.skip_src >= 0 ? (int)i - l.skip_src : l.Cout;
}

// shape, layer offsets, section offsets and body size of a body with `sections` for the layer table of `n`; everything else at its default
int fill_layout(const rcn_hipx_net& n, int sections, rcn_hipx_state_desc* d) {
    if ((int)n.L.size() > RCN_HIPX_STATE_MAX_LAYERS) return -3;
    *d = rcn_hipx_state_desc{};
    d->magic = RCN_HIPX_STATE_MAGIC; d->version = RCN_HIPX_STATE_VERSION;
    d->in_h = n.in_h; d->in_w = n.in_w; d->in_c = n.in_c; d->n_layers = (int)n.L.size();
    for (int i = 0; i < RCN_HIPX_STATE_MAX_LAYERS; ++i) d->layer_off[i] = -1;
    for (size_t i = 0; i < n.L.size(); ++i) {
        d->layers[i].kind = n.L[i].kind; d->layers[i].out = desc_out(n, i);
        if (n.L[i].row().params) d->layer_off[i] = n.L[i].lw_off;
    }
    d->classes = n.classes; d->n_log = n.n_log;
    d->precision = RCN_HIPX_FP32; d->tiling = RCN_HIPX_TILING_AUTO;
    d->sections = (sections & kStateAllSections) | RCN_HIPX_STATE_PARAMS;
    long long at = kStateScalarsBytes;
    for (int s = 0; s < kStateSections; ++s) {
        if (!(d->sections >> s & 1)) { d->section_off[s] = -1; continue; }
        d->section_off[s] = at;
        at += round256(n.n_log * (long long)sizeof(float));
    }
    d->body_bytes = at;
    const Recipe r{};
    d->optim = r.optim; d->sgd_nesterov = r.sgd_nesterov; d->sgd_momentum = r.sgd_mu; d->sgd_weight_decay = r.sgd_wd;
    d->adam_beta1 = r.adam_b1; d->adam_beta2 = r.adam_b2; d->adam_eps = r.adam_eps; d->adam_weight_decay = r.adam_wd; d->adam_decoupled = r.adam_decoupled;
    d->loss_eps = r.loss_eps; d->ema_decay = r.ema_decay; d->clip_max_norm = r.clip_max; d->accum_k = r.accum_k;
    d->dropout_p = r.drop_p; d->dropout_seed = r.drop_seed;
    return 0;
}

// the net's padded buffer of section s
Buf& section_buf(rcn_hipx_net* n, int s) {
    Buf* const b[kStateSections] = {&n->params, &n->vel, &n->adam_m, &n->adam_v, &n->ema, &n->accum};
    return *b[s];
}
const char* const kSectionName[kStateSections] = {"parameters", "velocity", "Adam m", "Adam v", "average", "accumulator"};

// The job table of a pack (units of logical elements) or an unpack (units of padded elements) over the sections of d.  The three scalar
// pointers are left for the caller.  false: more layers with parameters than one launch takes.
static_assert(kStateMaxJobs == kMaxReduceJobs, "describe_layers refuses by kMaxReduceJobs for both tables");
bool make_state_jobs(rcn_hipx_net* n, const rcn_hipx_state_desc& d, bool unpack, StateJobs* J) {
    *J = StateJobs{};
    int unit = 0;
    for (const Layer& l : n->L) {
        if (!l.row().params) continue;
        if (J->njobs == kStateMaxJobs) return false;
        StateJob& jb = J->j[J->njobs++];
        jb.pad_off = l.w_off; jb.log_off = l.lw_off;
        jb.n_pad = ((long long)l.K + 1) * l.CoutP; jb.n_log = ((long long)l.K + 1) * l.Cout;
        jb.Cout = l.Cout; jb.CoutP = l.CoutP;
        jb.vec = l.Cout == l.CoutP && l.w_off % 4 == 0 && l.lw_off % 4 == 0 && jb.n_log % 4 == 0;
        jb.first_unit = unit;
        unit += state_units(unpack ? jb.n_pad : jb.n_log);
    }
    J->units = unit;
    J->n_log = n->n_log; J->gap = (int)((round256(n->n_log * (long long)sizeof(float)) - n->n_log * (long long)sizeof(float)) / (long long)sizeof(float));
    for (int s = 0; s < kStateSections; ++s)
        if (d.sections >> s & 1) J->sec[J->nsec++] = StateSection{(float*)section_buf(n, s).p, d.section_off[s] / (long long)sizeof(float)};
    return true;
}
unsigned state_grid(const StateJobs& J) { const long long t = (long long)J.nsec * J.units; return (unsigned)(t < 1 ? 1 : t > kStateMaxBlocks ? kStateMaxBlocks : t); }

// nullptr, or why the recipe a descriptor carries is refused: the setters' own conditions, asked before anything changes
const char* recipe_refusal(const rcn_hipx_net* n, const rcn_hipx_state_desc& d) {
    if (d.optim != 0 && d.optim != 1) return "restore: the optimiser selected must be 0 (SGD) or 1 (Adam)";
    if (!(d.sgd_momentum >= 0.f && d.sgd_momentum < 1.f) || !(std::isfinite(d.sgd_weight_decay) && d.sgd_weight_decay >= 0.f) || (d.sgd_nesterov != 0 && d.sgd_nesterov != 1) ||
        (d.sgd_nesterov && d.sgd_momentum == 0.f)) return "restore: the SGD values are not ones rcn_hipx_set_sgd takes";
    if (!(d.adam_beta1 >= 0.f && d.adam_beta1 < 1.f && d.adam_beta2 >= 0.f && d.adam_beta2 < 1.f) || !(std::isfinite(d.adam_eps) && d.adam_eps > 0.f) ||
        !(std::isfinite(d.adam_weight_decay) && d.adam_weight_decay >= 0.f) || (d.adam_decoupled != 0 && d.adam_decoupled != 1)) return "restore: the Adam values are not ones rcn_hipx_set_adam takes";
    if (!(std::isfinite(d.loss_eps) && d.loss_eps >= 0.f && d.loss_eps < 1.f)) return "restore: the label smoothing is not one rcn_hipx_set_loss takes";
    if (!(std::isfinite(d.ema_decay) && d.ema_decay >= 0.f && d.ema_decay < 1.f)) return "restore: the decay is not one rcn_hipx_set_ema takes";
    if (!(d.clip_max_norm >= 0.f)) return "restore: the max norm is not one rcn_hipx_set_clip takes";
    if (d.accum_k < 1 || d.accum_k > 65536 || d.accum_pos < 0 || d.accum_pos >= d.accum_k) return "restore: k must be in 1 .. 65536 and the position in 0 .. k - 1";
    if (!(std::isfinite(d.dropout_p) && d.dropout_p >= 0.f && d.dropout_p < 1.f) || (d.dropout_p > 0.f && dropout_sites(n) == 0)) return "restore: the dropout rate is not one rcn_hipx_set_dropout takes for this net";
    return nullptr;
}

}  // namespace

extern "C" {

int rcn_hipx_state_desc_size(void) { return (int)sizeof(rcn_hipx_state_desc); }

int rcn_hipx_state_layout(int in_h, int in_w, int in_c, const rcn_hipx_layer* layers, int n_layers, int sections, rcn_hipx_state_desc* desc) {
    if (!layers || !desc || n_layers < 1 || in_h < 1 || in_w < 1 || in_c < 1 || sections < 0 || sections > kStateAllSections) return -1;
    if (n_layers > RCN_HIPX_STATE_MAX_LAYERS) return -3;
    rcn_hipx_net net;
    RTRY(make_dry_net(net, in_h, in_w, in_c, layers, n_layers, 1, RCN_HIPX_FP32, RCN_HIPX_TILING_AUTO));
    return fill_layout(net, sections, desc);
}

int rcn_hipx_snapshot_dev(rcn_hipx_net* n, int sections, void* body_dev, int64_t cap_bytes, rcn_hipx_state_desc* desc_out) {
    if (!n) return -1;
    if (!body_dev || !desc_out) return fail(n, -1, "snapshot: body_dev and desc_out must not be NULL");
    if (sections < 0 || sections > kStateAllSections) return fail(n, -1, "snapshot: unknown section bits");
    if ((uintptr_t)body_dev % 16 != 0) return fail(n, -1, "snapshot: the body must be 16-byte aligned");
    if (n->walk_open) return fail(n, -6, "snapshot: a bucket walk is open (rcn_hipx_gradients_begin_dev); take the remaining buckets first");
    int want = sections;
    if (want == 0)
        for (int s = 0; s < kStateSections; ++s) want |= section_buf(n, s).p ? 1 << s : 0;
    want |= RCN_HIPX_STATE_PARAMS;
    for (int s = 0; s < kStateSections; ++s)
        if ((want >> s & 1) && !section_buf(n, s).p) return fail(n, -6, std::string("snapshot: the net has no ") + kSectionName[s] + " buffer");
    rcn_hipx_state_desc d;
    if (fill_layout(*n, want, &d) != 0) return fail(n, -3, "snapshot: the net has more layers than a descriptor holds (RCN_HIPX_STATE_MAX_LAYERS)");
    if (cap_bytes < d.body_bytes) return fail(n, -1, "snapshot: cap_bytes is smaller than the body (rcn_hipx_state_layout gives body_bytes)");
    StateJobs J;
    if (!make_state_jobs(n, d, false, &J)) return fail(n, -3, "snapshot: more layers with parameters than one launch takes");
    d.precision = n->store16 ? RCN_HIPX_BF16_STORED : n->precision; d.tiling = n->tiling;
    d.flags = RCN_HIPX_STATE_HAS_RECIPE | (n->adam_tick.p ? RCN_HIPX_STATE_HAS_ADAM_TICK : 0) | (n->drop_tick.p ? RCN_HIPX_STATE_HAS_DROPOUT_TICK : 0) | (n->clip_state.p ? RCN_HIPX_STATE_HAS_CLIP_STATE : 0);
    d.accum_pos = n->accum_pos;
    d.optim = n->optim; d.sgd_nesterov = n->sgd_nesterov; d.sgd_momentum = n->sgd_mu; d.sgd_weight_decay = n->sgd_wd;
    d.adam_beta1 = n->adam_b1; d.adam_beta2 = n->adam_b2; d.adam_eps = n->adam_eps; d.adam_weight_decay = n->adam_wd; d.adam_decoupled = n->adam_decoupled;
    d.loss_eps = n->loss_eps; d.ema_decay = n->ema_decay; d.clip_max_norm = n->clip_max; d.accum_k = n->accum_k;
    d.dropout_p = n->drop_p; d.dropout_seed = (uint64_t)n->drop_seed;
    J.tick = (unsigned*)n->adam_tick.p; J.drop = (unsigned*)n->drop_tick.p; J.clip = (unsigned*)n->clip_state.p;
    Dev g(n->device);
    hipLaunchKernelGGL(k_state_pack, dim3(state_grid(J)), dim3(kStateThreads), 0, n->stream, J, (float*)body_dev);
    XTRY(n, hipGetLastError());
    *desc_out = d;
    return 0;
}

int rcn_hipx_restore_dev(rcn_hipx_net* n, const rcn_hipx_state_desc* desc, const void* body_dev, int64_t body_bytes) {
    if (!n) return -1;
    if (!desc || !body_dev) return fail(n, -1, "restore: desc and body_dev must not be NULL");
    const rcn_hipx_state_desc d = *desc;
    // ---- everything is checked on the host before anything changes
    if (d.magic != RCN_HIPX_STATE_MAGIC || d.version != RCN_HIPX_STATE_VERSION) return fail(n, -1, "restore: not a state descriptor of this version (magic, version)");
    if ((uintptr_t)body_dev % 16 != 0) return fail(n, -1, "restore: the body must be 16-byte aligned");
    if (d.n_layers < 1 || d.n_layers > RCN_HIPX_STATE_MAX_LAYERS) return fail(n, -1, "restore: the descriptor's layer count is out of range");
    if (d.sections < 0 || d.sections > kStateAllSections || !(d.sections & RCN_HIPX_STATE_PARAMS)) return fail(n, -1, "restore: the section mask must hold the parameters and no unknown bit");
    if (d.flags < 0 || d.flags > 15) return fail(n, -1, "restore: unknown flag bits");
    if (d.in_h != n->in_h || d.in_w != n->in_w || d.in_c != n->in_c || d.n_layers != (int)n->L.size() || d.n_log != n->n_log || d.classes != n->classes)
        return fail(n, -2, "restore: the descriptor's input shape, layer count or parameter count is not this net's");
    for (int i = 0; i < d.n_layers; ++i) {
        const Layer& l = n->L[i];
        if (d.layers[i].kind != l.kind || (l.row().params && d.layers[i].out != desc_out(*n, (size_t)i))) return fail(n, -2, "restore: the descriptor's layer list is not this net's");
    }
    const long long sec_bytes = n->n_log * (long long)sizeof(float);
    if (d.body_bytes < kStateScalarsBytes || body_bytes < d.body_bytes) return fail(n, -1, "restore: body_bytes is smaller than the body the descriptor describes");
    for (int s = 0; s < kStateSections; ++s) {
        if (!(d.sections >> s & 1)) continue;
        const long long off = d.section_off[s];
        if (off < kStateScalarsBytes || off % 256 != 0 || off > d.body_bytes - sec_bytes) return fail(n, -1, "restore: a section lies outside the body or is not 256-byte aligned");
    }
    if (d.precision != RCN_HIPX_FP32 && d.precision != RCN_HIPX_BF16 && d.precision != RCN_HIPX_BF16_STORED) return fail(n, -1, "restore: unknown precision mode");
    if (d.tiling != RCN_HIPX_TILING_GEMM && d.tiling != RCN_HIPX_TILING_AUTO && d.tiling != RCN_HIPX_TILING_LDS) return fail(n, -1, "restore: unknown tiling mode");
    const bool has_recipe = d.flags & RCN_HIPX_STATE_HAS_RECIPE;
    if (has_recipe) if (const char* why = recipe_refusal(n, d)) return fail(n, -1, why);
    if (d.precision == RCN_HIPX_BF16_STORED && !n->store16) {
        std::string why;
        rcn_hipx_net probe;                             // (the tiling the restore is about to set decides which kernels run)
        make_dry_net(probe, *n, n->max_batch);
        probe.tiling = d.tiling;
        const int ps = store16_covered(probe, &why);
        if (ps != 0) return fail(n, ps, why);
    }
    if (n->walk_open) return fail(n, -6, "restore: a bucket walk is open (rcn_hipx_gradients_begin_dev); take the remaining buckets first");
    StateJobs J;
    if (!make_state_jobs(n, d, true, &J)) return fail(n, -3, "restore: more layers with parameters than one launch takes");
    // ---- precision, tiling and the recipe through the setters: each allocates, synchronises and drops the graphs exactly where it always
    // does, and none is called for a setting the net already has (a restore into a net with the same settings drops no graph)
    Dev g(n->device);
    RTRY(rcn_hipx_set_tiling(n, d.tiling));
    RTRY(rcn_hipx_set_precision(n, d.precision));
    if (has_recipe) {
        if (d.sgd_momentum != n->sgd_mu || d.sgd_weight_decay != n->sgd_wd || d.sgd_nesterov != n->sgd_nesterov) RTRY(rcn_hipx_set_sgd(n, d.sgd_momentum, d.sgd_weight_decay, d.sgd_nesterov));
        if (d.adam_beta1 != n->adam_b1 || d.adam_beta2 != n->adam_b2 || d.adam_eps != n->adam_eps || d.adam_weight_decay != n->adam_wd || d.adam_decoupled != n->adam_decoupled ||
            (d.optim == 1 && (n->optim != 1 || !n->adam_tick.p)))
            RTRY(rcn_hipx_set_adam(n, d.adam_beta1, d.adam_beta2, d.adam_eps, d.adam_weight_decay, d.adam_decoupled));
        if (d.optim == 0 && n->optim != 0) RTRY(rcn_hipx_set_sgd(n, d.sgd_momentum, d.sgd_weight_decay, d.sgd_nesterov));      // (SGD selected again)
        RTRY(rcn_hipx_set_loss(n, d.loss_eps));
        RTRY(rcn_hipx_set_ema(n, d.ema_decay));
        RTRY(rcn_hipx_set_clip(n, d.clip_max_norm));
        RTRY(rcn_hipx_set_accumulate(n, d.accum_k));
        RTRY(rcn_hipx_set_dropout(n, d.dropout_p, d.dropout_seed));
    }
    // ---- the buffers of what the snapshot carries and the recipe leaves switched off (a velocity under Adam, an average with decay 0):
    // allocated once, like every buffer behind the recipe
    const bool has_tick = d.flags & RCN_HIPX_STATE_HAS_ADAM_TICK, has_drop = d.flags & RCN_HIPX_STATE_HAS_DROPOUT_TICK, has_clip = d.flags & RCN_HIPX_STATE_HAS_CLIP_STATE;
    bool missing = (has_tick && !n->adam_tick.p) || (has_drop && !n->drop_tick.p) || (has_clip && !n->clip_state.p);
    for (int s = 1; s < kStateSections; ++s) missing = missing || ((d.sections >> s & 1) && !section_buf(n, s).p);
    if (missing)
        RTRY(reconfigure(n, {{(d.sections & RCN_HIPX_STATE_VELOCITY) != 0, &n->vel, padded_bytes(n), nullptr}, {(d.sections & RCN_HIPX_STATE_ADAM_M) != 0, &n->adam_m, padded_bytes(n), nullptr},
                             {(d.sections & RCN_HIPX_STATE_ADAM_V) != 0, &n->adam_v, padded_bytes(n), nullptr}, {(d.sections & RCN_HIPX_STATE_EMA) != 0, &n->ema, padded_bytes(n), n->params.p},
                             {(d.sections & RCN_HIPX_STATE_ACCUM) != 0, &n->accum, padded_bytes(n), nullptr}, {has_tick, &n->adam_tick, sizeof(AdamTick), nullptr},
                             {has_drop, &n->drop_tick, sizeof(long long), nullptr}, {has_clip, &n->clip_state, (size_t)kStateClipBytes, nullptr}}));
    if (has_recipe) n->accum_pos = d.accum_pos;
    // ---- the one unpack launch, then the tap-flipped copy from the restored parameters (the bf16 operand copies are re-made by the next step)
    make_state_jobs(n, d, true, &J);                    // (again: the buffers above may be new)
    J.tick = has_tick ? (unsigned*)n->adam_tick.p : nullptr; J.drop = has_drop ? (unsigned*)n->drop_tick.p : nullptr; J.clip = has_clip ? (unsigned*)n->clip_state.p : nullptr;
    hipLaunchKernelGGL(k_state_unpack, dim3(state_grid(J)), dim3(kStateThreads), 0, n->stream, J, (const float*)body_dev);
    XTRY(n, hipGetLastError());
    return refresh_flipped(n);
}

int rcn_hipx_set_accumulated(rcn_hipx_net* n, const float* flat, int pending) {
    if (!n || !flat) return -1;
    if (n->accum_k == 1 || !n->accum.p) return fail(n, -6, "set_accumulated: the net does not accumulate (rcn_hipx_set_accumulate with k > 1 first)");
    if (pending < 0 || pending >= n->accum_k) return fail(n, -1, "set_accumulated: pending must be in 0 .. k - 1");
    Dev g(n->device);
    RTRY(upload_padded(n, n->accum, flat));
    n->accum_pos = pending;
    return 0;
}

}  // extern "C"
