// rcn_hipx_api_dropout.ipp -- part of rcn_hipx_api.hip (one translation unit): the entry points of dropout (convnet_dropout.hpp).  The
// launches themselves sit beside the forward and backward walks (launch_dropout_tick / _fwd / _bwd, rcn_hipx_api.hip).

namespace {

// the host constants of a rate p (finite, 0 <= p < 1)
float dropout_scale(float p) { const float q = 1.0f - p; return 1.0f / q; }
unsigned dropout_threshold(float p) { return (unsigned)llrint((double)p * 16777216.0); }

// the ordinal's buffer, zeroed, outside any capture; the stream idle afterwards.  No graph holds its pointer before it exists.
int ensure_drop_tick(rcn_hipx_net* n) {
    if (n->drop_tick.p) return 0;
    XTRY(n, hipStreamSynchronize(n->stream));
    XTRY(n, n->drop_tick.ensure(sizeof(long long)));
    XTRY(n, hipMemsetAsync(n->drop_tick.p, 0, sizeof(long long), n->stream));
    XTRY(n, hipStreamSynchronize(n->stream));
    return 0;
}

}  // namespace

extern "C" {

int rcn_hipx_set_dropout(rcn_hipx_net* n, float p, uint64_t seed) {
    if (!n) return -1;
    if (!(std::isfinite(p) && p >= 0.f && p < 1.f)) return fail(n, -1, "set_dropout: p must be finite and in [0, 1)");
    if (p == 0.f) p = 0.f;                              // (-0)
    if (p > 0.f && dropout_sites(n) == 0) return fail(n, -3, std::string("set_dropout: the net has no ") + kind_row(RCN_HIPX_DENSE_RELU).name + " layer to drop behind");
    if (p == n->drop_p && (unsigned long long)seed == n->drop_seed) return 0;
    Dev g(n->device);
    RTRY(reconfigure(n, {{p != 0.f, &n->drop_tick, sizeof(long long), nullptr}}));
    n->drop_p = p; n->drop_seed = (unsigned long long)seed; n->drop_s = dropout_scale(p); n->drop_thr = dropout_threshold(p);
    return 0;
}

int rcn_hipx_get_dropout(const rcn_hipx_net* n, float* p, uint64_t* seed, int* sites) {
    if (!n) return -1;
    if (p) *p = n->drop_p;
    if (seed) *seed = (uint64_t)n->drop_seed;
    if (sites) *sites = dropout_sites(n);
    return 0;
}

int rcn_hipx_get_dropout_state(rcn_hipx_net* n, int64_t* forwards) {
    if (!n || !forwards) return -1;
    Dev g(n->device);
    long long t = 0;
    if (n->drop_tick.p) XTRY(n, hipMemcpyAsync(&t, n->drop_tick.p, sizeof t, hipMemcpyDeviceToHost, n->stream));
    XTRY(n, hipStreamSynchronize(n->stream));
    *forwards = (int64_t)t;
    return 0;
}

int rcn_hipx_set_dropout_state(rcn_hipx_net* n, int64_t forwards) {
    if (!n) return -1;
    if (forwards < 0) return fail(n, -1, "set_dropout_state: forwards must be >= 0");
    Dev g(n->device);
    RTRY(ensure_drop_tick(n));
    const long long t = (long long)forwards;
    XTRY(n, hipMemcpyAsync(n->drop_tick.p, &t, sizeof t, hipMemcpyHostToDevice, n->stream));
    XTRY(n, hipStreamSynchronize(n->stream));
    return 0;
}

int rcn_hipx_dropout_draw(float p, uint64_t seed, uint64_t t, int site, uint64_t idx, int* keep) {
    if (!keep || !(std::isfinite(p) && p >= 0.f && p < 1.f) || site < 0 || site > 0xffff) return -1;
    *keep = dropout_keep(dropout_stem((unsigned long long)seed, (unsigned long long)t), ((unsigned long long)site << 48) + (unsigned long long)idx, dropout_threshold(p)) ? 1 : 0;
    return 0;
}

int rcn_hipx_dropout_apply_dev(rcn_hipx_net* n, int site, int64_t t, float* a, int B) {
    if (!n) return -1;
    if (!a || (uintptr_t)a % 16 != 0) return fail(n, -1, "dropout_apply: a 16-byte aligned device buffer of B x units floats");
    if (site < 0 || site >= dropout_sites(n)) return fail(n, -1, "dropout_apply: no such site (rcn_hipx_get_dropout reports their number)");
    RTRY(ensure_batch(n, B));
    int U = 0, d = 0;
    for (const Layer& l : n->L)
        if (l.kind == RCN_HIPX_DENSE_RELU && d++ == site) U = l.CoutP;
    Dev g(n->device);
    return launch_dropout_fwd(n, site, a, B, U, nullptr, (long long)t);
}

}  // extern "C"
