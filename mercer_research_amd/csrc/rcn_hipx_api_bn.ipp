// rcn_hipx_api_bn.ipp -- part of rcn_hipx_api.hip (one translation unit): the entry points of batch normalisation (convnet_bn.hpp; the
// launches are launch_bn_forward / launch_bn_backward beside the layer walks): momentum and eps, and the running statistics to and from
// the host -- all RCN_HIPX_BN_RELU and RCN_HIPX_BN_ADD_RELU layers (the kinds whose row says bn: convnet_kinds.hpp) back to back, mean[C] then var[C] per layer.

extern "C" {

int rcn_hipx_set_bn(rcn_hipx_net* n, float momentum, float eps) {
    if (!n) return -1;
    if (!(std::isfinite(momentum) && momentum >= 0.f && momentum <= 1.f)) return fail(n, -1, "set_bn: momentum must be finite and in [0, 1]");
    if (!(std::isfinite(eps) && eps > 0.f)) return fail(n, -1, "set_bn: eps must be finite and > 0");
    if (momentum == n->bn_momentum && eps == n->bn_eps) return 0;
    const Recipe defaults{};
    if (bn_layers(n) == 0 && (momentum != defaults.bn_momentum || eps != defaults.bn_eps)) return fail(n, -3, std::string("set_bn: the net has no ") + kind_row(RCN_HIPX_BN_RELU).name + " layer");
    Dev g(n->device);
    RTRY(reconfigure(n));                               // (captured graphs bake in the two values: kernel arguments)
    n->bn_momentum = momentum; n->bn_eps = eps;
    return 0;
}

int rcn_hipx_get_bn(const rcn_hipx_net* n, float* momentum, float* eps, int* layers) {
    if (!n) return -1;
    if (momentum) *momentum = n->bn_momentum;
    if (eps) *eps = n->bn_eps;
    if (layers) *layers = bn_layers(n);
    return 0;
}

int rcn_hipx_bn_stats_count(const rcn_hipx_net* n, int64_t* floats) {
    if (!n || !floats) return -1;
    int64_t c = 0;
    for (const Layer& l : n->L) if (l.row().bn) c += 2 * (int64_t)l.Cout;
    *floats = c;
    return 0;
}

int rcn_hipx_get_bn_stats(rcn_hipx_net* n, float* stats) {
    if (!n || !stats) return -1;
    Dev g(n->device);
    float* at = stats;
    for (const Layer& l : n->L) {
        if (!l.row().bn) continue;
        XTRY(n, hipMemcpyAsync(at, bn_run_mean(l), (size_t)2 * l.Cout * sizeof(float), hipMemcpyDeviceToHost, n->stream));      // [running mean | running var] are adjacent
        at += 2 * l.Cout;
    }
    XTRY(n, hipStreamSynchronize(n->stream));
    return 0;
}

int rcn_hipx_set_bn_stats(rcn_hipx_net* n, const float* stats) {
    if (!n || !stats) return -1;
    Dev g(n->device);
    const float* at = stats;
    for (const Layer& l : n->L) {
        if (!l.row().bn) continue;
        XTRY(n, hipMemcpyAsync(bn_run_mean(l), at, (size_t)2 * l.Cout * sizeof(float), hipMemcpyHostToDevice, n->stream));
        at += 2 * l.Cout;
    }
    XTRY(n, hipStreamSynchronize(n->stream));
    return 0;
}

int rcn_hipx_bn_partials(int64_t rows, int* parts, int* capacity) {
    if (rows < 1 || !parts || !capacity) return -1;
    *parts = bn_parts((long long)rows);
    *capacity = bn_parts_cap((long long)rows);
    return 0;
}

int rcn_hipx_reset_bn_stats(rcn_hipx_net* n) {
    if (!n) return -1;
    Dev g(n->device);
    return bn_reset_stats(n);
}

}  // extern "C"
