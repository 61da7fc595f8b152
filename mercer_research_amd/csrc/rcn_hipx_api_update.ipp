// rcn_hipx_api_update.ipp -- part of rcn_hipx_api.hip (one translation unit): the update path.  The step's reduction launches
// (run_reduce_jobs: choose -- select_update, convnet_select.hpp --, make the tables, note the plan or launch) and the entry points of the
// optimisers (SGD, Adam), the loss, the average, clipping and accumulation, with the data-parallel half (rcn_hipx_apply_sgd_dev).

namespace {

SgdParams sgd_params(const rcn_hipx_net* n) { return SgdParams{(float*)n->vel.p, (const float*)n->params.p, n->sgd_mu, n->sgd_wd, n->sgd_nesterov}; }
AdamParams adam_params(const rcn_hipx_net* n) {
    return AdamParams{(float*)n->adam_m.p, (float*)n->adam_v.p, (const float*)n->params.p, (const AdamTick*)n->adam_tick.p,
                      n->adam_b1, n->adam_b2, n->adam_a1, n->adam_a2, n->adam_eps, n->adam_wd, n->adam_decoupled};
}
// the update's ordinal and its bias corrections advance on the device, directly in front of the launch that reads them (convnet_adam.hpp)
void launch_adam_tick(rcn_hipx_net* n) { hipLaunchKernelGGL(k_adam_tick, dim3(1), dim3(1), 0, n->stream, (AdamTick*)n->adam_tick.p, n->adam_b1, n->adam_b2); }
// the tick state after `step` updates, by the device's own arithmetic
AdamTick adam_tick_at(long long step, float b1, float b2) {
    AdamTick t{0, 1.0, 1.0, 0.f, 0.f};
    while (t.step < step) {
        const AdamTick before = t;
        adam_tick(t, b1, b2);
        if (t.b1t == before.b1t && t.b2t == before.b2t) t.step = step;      // both products at their fixed point: every later tick only counts
    }
    return t;
}
EmaParams ema_params(const rcn_hipx_net* n) { return EmaParams{(float*)n->ema.p, (const float*)n->params.p, 1.0f - n->ema_decay}; }
// the clipped launch's view of the net's clip state; the partials are those of the buffer k_grad_sumsq has just summed
ClipParams clip_params(const rcn_hipx_net* n) {
    unsigned long long* const count = (unsigned long long*)n->clip_state.p;
    return ClipParams{(const double*)n->clip_part.p, (int)clip_blocks(n->n_pad), n->clip_max, (float*)(count + 1), n->clip_log, n->clip_log_cap, count};
}
// partial[b] of every 4096-element block of g[0, len) (len % 4 == 0, g 16-byte aligned), on the net's stream
void launch_sumsq(rcn_hipx_net* n, const float* g, long long len, float scale, double* partial) {
    if (len > 0) hipLaunchKernelGGL(k_grad_sumsq, dim3((unsigned)clip_blocks(len)), dim3(kClipThreads), 0, n->stream, g, len, scale, partial);
}

// The tables of a step's reduction, made from the queued jobs (which stay as they are).  Not buffered: `update` is the one launch, the
// queued jobs with the rate.  Buffered (accumulation, clipping: convnet_accum.hpp, convnet_clip.hpp): `first` is the launch that leaves the
// summed gradient in `summed`, a buffer laid out like the parameters -- k_reduce_all_acc, each job's "parameters" being its layer's slice
// of the accumulator, or the gradients-only reduction into the net's gradient buffer; neither has a flipped copy -- and `update` the
// launch over that buffer, each job reading its layer's slice as a one-chunk slab, so the flipped weight copy, the velocity and the
// average are kept as the unbuffered launch keeps them.
struct ReduceTables { ReduceJobs first, update; long long blocks; int ublocks; };      // workgroups over the queued slabs / of a buffered update
ReduceTables make_tables(const ReduceJobs& queued, const UpdateChoice& c, float lr, const float* params, float* summed) {
    const ReduceJob& last = queued.j[queued.njobs - 1];
    ReduceTables t;
    t.blocks = last.first_block + (last.n + reduce_job_elems(last.chunks) - 1) / reduce_job_elems(last.chunks);
    t.ublocks = 0;
    t.update = queued;
    t.update.lr = lr; t.update.apply = c.update ? 1 : 0;
    if (!c.buffered) return t;                          // (`first` is not made: nothing launches it)
    t.first = queued;
    t.first.lr = 0.f; t.first.apply = c.acc ? 1 : 0;
    for (int q = 0; q < queued.njobs; ++q) {
        ReduceJob& f = t.first.j[q];
        ReduceJob& u = t.update.j[q];
        float* const slice = summed + (f.p - params);
        if (c.acc) { f.p = slice; f.grad = nullptr; } else f.grad = slice;
        f.flip.wt = nullptr;
        u.grad = nullptr;
        u.slab = slice;
        u.chunks = 1;
        u.first_block = t.ublocks;
        t.ublocks += (int)((u.n + reduce_job_elems(1) - 1) / reduce_job_elems(1));
    }
    return t;
}

int launch_reduction(rcn_hipx_net* n, const UpdateChoice& c, const ReduceTables& t, const float* summed, const float* lr_dev) {
    const dim3 block(kReduceThreads), grid((unsigned)t.blocks);
    if (c.acc) {
        with_bool(c.first, [&](auto FIRST) { hipLaunchKernelGGL(k_reduce_all_acc<decltype(FIRST)::value>, grid, block, 0, n->stream, t.first, n->accum_c); });
        XTRY(n, hipGetLastError());
        if (!c.update) return 0;
    } else if (c.clip) {
        hipLaunchKernelGGL((k_reduce_update<false, kOptPlain, false, false>), grid, block, 0, n->stream, t.first, UpdateArgs<false, kOptPlain, false, false>{});
        XTRY(n, hipGetLastError());
    }
    if (c.clip) {
        launch_sumsq(n, summed, n->n_pad, 1.0f, (double*)n->clip_part.p);
        XTRY(n, hipGetLastError());
    }
    if (c.adam) {
        launch_adam_tick(n);
        XTRY(n, hipGetLastError());
    }
    // gradients-only walks (apply == false) take the plain form
    const dim3 ugrid(c.buffered ? (unsigned)t.ublocks : (unsigned)t.blocks);
    with_bool(c.clip, [&](auto CLIP) { with_const<kOptAdam, kOptSgd, kOptPlain>(c.adam ? kOptAdam : c.sgd ? kOptSgd : kOptPlain, [&](auto OPT) { with_bool(c.ema, [&](auto EMA) { with_bool(c.dlr, [&](auto DLR) {
        constexpr bool clip = decltype(CLIP)::value, ema = decltype(EMA)::value, dlr = decltype(DLR)::value;
        constexpr int opt = decltype(OPT)::value;
        UpdateArgs<clip, opt, ema, dlr> A{};            // the form's own argument list: what it reads
        if constexpr (opt == kOptSgd) A.opt() = sgd_params(n);
        if constexpr (opt == kOptAdam) A.opt() = adam_params(n);
        if constexpr (ema) A.ema() = ema_params(n);
        if constexpr (clip) A.clip() = clip_params(n);
        if constexpr (dlr) A.lr() = lr_dev;
        hipLaunchKernelGGL((k_reduce_update<clip, opt, ema, dlr>), ugrid, block, 0, n->stream, t.update, A);
    }); }); }); });
    XTRY(n, hipGetLastError());
    return 0;
}

int run_reduce_jobs(rcn_hipx_net* n, float lr, bool apply, const float* lr_dev, int micro) {
    if (!n->jobs.njobs) return 0;
    const UpdateChoice c = select_update(*n, apply, micro, lr_dev != nullptr);
    float* const summed = (float*)(c.acc ? n->accum.p : n->clip_grad.p);      // (a dry run has no buffers)
    const ReduceTables t = make_tables(n->jobs, c, lr, (const float*)n->params.p, summed);
    if (n->dry) n->plan += describe_update(c, *n, n->jobs.njobs, t.blocks, t.ublocks, n->n_pad, clip_blocks(n->n_pad));
    else RTRY(launch_reduction(n, c, t, summed, lr_dev));
    n->jobs.njobs = 0;
    return 0;
}

// What the setters share: the stream idle; each of `fresh` that is needed now and does not exist yet allocated and filled -- with zeros,
// or with a copy of `bytes` bytes of `like` -- once and outside any capture (captured graphs hold these pointers, so the buffers never
// move afterwards), and the stream idle again; the graphs dropped (they bake in the update's launches and their arguments).
struct Fresh { bool needed; Buf* buf; size_t bytes; const void* like; };
int reconfigure(rcn_hipx_net* n, std::initializer_list<Fresh> fresh = {}) {
    XTRY(n, hipStreamSynchronize(n->stream));
    for (const Fresh& f : fresh) {
        if (!f.needed || f.buf->p) continue;
        XTRY(n, f.buf->ensure(f.bytes));
        if (f.like) XTRY(n, hipMemcpyAsync(f.buf->p, f.like, f.bytes, hipMemcpyDeviceToDevice, n->stream));
        else XTRY(n, hipMemsetAsync(f.buf->p, 0, f.bytes, n->stream));
    }
    XTRY(n, hipStreamSynchronize(n->stream));
    drop_graphs(n);
    return 0;
}
size_t padded_bytes(const rcn_hipx_net* n) { return (size_t)n->n_pad * sizeof(float); }

}  // namespace

extern "C" {

__global__ void k_axpy(float* __restrict__ p, const float* __restrict__ g, float scale, long long n) {
    for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (long long)gridDim.x * blockDim.x) p[i] = p[i] - scale * g[i];
}

// p <- p - scale * g over the padded parameters
static int launch_axpy(rcn_hipx_net* n, const float* grad, float scale) {
    hipLaunchKernelGGL(k_axpy, dim3(grid1d(n->n_pad, 256)), dim3(256), 0, n->stream, (float*)n->params.p, grad, scale, n->n_pad);
    XTRY(n, hipGetLastError());
    return 0;
}

int rcn_hipx_apply_dev(rcn_hipx_net* n, const float* grad, float scale) {
    if (!n || !grad) return -1;
    Dev g(n->device);
    RTRY(launch_axpy(n, grad, scale));
    return refresh_flipped(n);                          // (the plain axpy: neither the velocity nor the average moves)
}

int rcn_hipx_set_sgd(rcn_hipx_net* n, float momentum, float weight_decay, int nesterov) {
    if (!n) return -1;
    if (!(momentum >= 0.f && momentum < 1.f)) return fail(n, -1, "set_sgd: momentum must be in [0, 1)");
    if (!(std::isfinite(weight_decay) && weight_decay >= 0.f)) return fail(n, -1, "set_sgd: weight_decay must be finite and >= 0");
    if (nesterov != 0 && nesterov != 1) return fail(n, -1, "set_sgd: nesterov must be 0 or 1");
    if (nesterov && momentum == 0.f) return fail(n, -1, "set_sgd: nesterov needs a momentum > 0");
    if (!adam_on(*n) && momentum == n->sgd_mu && weight_decay == n->sgd_wd && nesterov == n->sgd_nesterov) return 0;
    Dev g(n->device);
    RTRY(reconfigure(n, {{momentum != 0.f, &n->vel, padded_bytes(n), nullptr}}));
    n->sgd_mu = momentum; n->sgd_wd = weight_decay; n->sgd_nesterov = nesterov;
    n->optim = 0;                                       // (SGD selected again: Adam's moments and tick stay as they are)
    return 0;
}

// the tick state to and from the host, behind whatever the stream still holds
static int read_adam_tick(rcn_hipx_net* n, AdamTick* t) {
    XTRY(n, hipMemcpyAsync(t, n->adam_tick.p, sizeof *t, hipMemcpyDeviceToHost, n->stream));
    XTRY(n, hipStreamSynchronize(n->stream));
    return 0;
}
static int write_adam_tick(rcn_hipx_net* n, const AdamTick& t) {
    XTRY(n, hipMemcpyAsync(n->adam_tick.p, &t, sizeof t, hipMemcpyHostToDevice, n->stream));
    XTRY(n, hipStreamSynchronize(n->stream));
    return 0;
}

int rcn_hipx_set_adam(rcn_hipx_net* n, float beta1, float beta2, float eps, float weight_decay, int decoupled) {
    if (!n) return -1;
    if (!(beta1 >= 0.f && beta1 < 1.f && beta2 >= 0.f && beta2 < 1.f)) return fail(n, -1, "set_adam: the betas must be in [0, 1)");
    if (!(std::isfinite(eps) && eps > 0.f)) return fail(n, -1, "set_adam: eps must be finite and > 0");
    if (!(std::isfinite(weight_decay) && weight_decay >= 0.f)) return fail(n, -1, "set_adam: weight_decay must be finite and >= 0");
    if (decoupled != 0 && decoupled != 1) return fail(n, -1, "set_adam: decoupled must be 0 or 1");
    Dev g(n->device);
    const bool fresh = !n->adam_tick.p;
    RTRY(reconfigure(n, {{true, &n->adam_m, padded_bytes(n), nullptr}, {true, &n->adam_v, padded_bytes(n), nullptr}, {true, &n->adam_tick, sizeof(AdamTick), nullptr}}));
    if (fresh) RTRY(write_adam_tick(n, adam_tick_at(0, beta1, beta2)));
    else if (beta1 != n->adam_b1 || beta2 != n->adam_b2) {
        // the running products belong to the betas: rebuilt from the update count, as the device would have made them
        AdamTick t;
        RTRY(read_adam_tick(n, &t));
        if (t.step > 0) RTRY(write_adam_tick(n, adam_tick_at(t.step, beta1, beta2)));
    }
    n->adam_b1 = beta1; n->adam_b2 = beta2; n->adam_a1 = 1.0f - beta1; n->adam_a2 = 1.0f - beta2;
    n->adam_eps = eps; n->adam_wd = weight_decay; n->adam_decoupled = decoupled;
    n->optim = 1;
    return 0;
}

int rcn_hipx_get_adam(const rcn_hipx_net* n, float* beta1, float* beta2, float* eps, float* weight_decay, int* decoupled, int* selected) {
    if (!n) return -1;
    if (beta1) *beta1 = n->adam_b1;
    if (beta2) *beta2 = n->adam_b2;
    if (eps) *eps = n->adam_eps;
    if (weight_decay) *weight_decay = n->adam_wd;
    if (decoupled) *decoupled = n->adam_decoupled;
    if (selected) *selected = adam_on(*n) ? 1 : 0;
    return 0;
}

int rcn_hipx_get_adam_state(rcn_hipx_net* n, float* m_flat, float* v_flat, int64_t* step) {
    if (!n) return -1;
    if (!n->adam_tick.p) return fail(n, -6, "get_adam_state: the net has no Adam state (rcn_hipx_set_adam first)");
    Dev g(n->device);
    if (m_flat) RTRY(unpad(n, (const float*)n->adam_m.p, m_flat));
    if (v_flat) RTRY(unpad(n, (const float*)n->adam_v.p, v_flat));
    if (step) {
        AdamTick t;
        RTRY(read_adam_tick(n, &t));
        *step = (int64_t)t.step;
    }
    return 0;
}

int rcn_hipx_set_adam_state(rcn_hipx_net* n, const float* m_flat, const float* v_flat, int64_t step) {
    if (!n || !m_flat || !v_flat) return -1;
    if (!n->adam_tick.p) return fail(n, -6, "set_adam_state: the net has no Adam state (rcn_hipx_set_adam first)");
    if (step < 0) return fail(n, -1, "set_adam_state: step must be >= 0");
    Dev g(n->device);
    RTRY(upload_padded(n, n->adam_m, m_flat));
    RTRY(upload_padded(n, n->adam_v, v_flat));
    return write_adam_tick(n, adam_tick_at((long long)step, n->adam_b1, n->adam_b2));      // b1t, b2t, c1, c2 rebuilt from the count
}

int rcn_hipx_reset_adam(rcn_hipx_net* n) {
    if (!n) return -1;
    if (!n->adam_tick.p) return 0;
    Dev g(n->device);
    XTRY(n, hipMemsetAsync(n->adam_m.p, 0, padded_bytes(n), n->stream));
    XTRY(n, hipMemsetAsync(n->adam_v.p, 0, padded_bytes(n), n->stream));
    return write_adam_tick(n, adam_tick_at(0, n->adam_b1, n->adam_b2));
}

int rcn_hipx_set_loss(rcn_hipx_net* n, float label_smoothing) {
    if (!n) return -1;
    if (!(std::isfinite(label_smoothing) && label_smoothing >= 0.f && label_smoothing < 1.f)) return fail(n, -1, "set_loss: label_smoothing must be finite and in [0, 1)");
    if (label_smoothing == n->loss_eps) return 0;
    Dev g(n->device);
    RTRY(reconfigure(n));                               // (captured graphs bake in the loss kernel and its arguments)
    n->loss_eps = label_smoothing;
    return 0;
}

int rcn_hipx_get_loss(const rcn_hipx_net* n, float* label_smoothing) {
    if (!n) return -1;
    if (label_smoothing) *label_smoothing = n->loss_eps;
    return 0;
}

int rcn_hipx_get_sgd(const rcn_hipx_net* n, float* momentum, float* weight_decay, int* nesterov) {
    if (!n) return -1;
    if (momentum) *momentum = n->sgd_mu;
    if (weight_decay) *weight_decay = n->sgd_wd;
    if (nesterov) *nesterov = n->sgd_nesterov;
    return 0;
}

int rcn_hipx_get_velocity(rcn_hipx_net* n, float* flat) {
    if (!n || !flat) return -1;
    if (!n->vel.p) { std::memset(flat, 0, (size_t)n->n_log * sizeof(float)); return 0; }
    Dev g(n->device);
    return unpad(n, (const float*)n->vel.p, flat);
}

int rcn_hipx_set_velocity(rcn_hipx_net* n, const float* flat) {
    if (!n || !flat) return -1;
    if (n->sgd_mu == 0.f || !n->vel.p) return fail(n, -6, "set_velocity: the net has no momentum (rcn_hipx_set_sgd first)");
    Dev g(n->device);
    return upload_padded(n, n->vel, flat);
}

int rcn_hipx_reset_velocity(rcn_hipx_net* n) {
    if (!n) return -1;
    if (!n->vel.p) return 0;
    Dev g(n->device);
    XTRY(n, hipMemsetAsync(n->vel.p, 0, padded_bytes(n), n->stream));
    return 0;
}

// the average follows the parameters that rcn_hipx_apply_sgd_dev's update launch has just stored (one more launch: this path is not the
// captured step, and it leaves the update launches exactly what they are without an average)
static int apply_ema(rcn_hipx_net* n) {
    if (!ema_on(*n)) return 0;
    const EmaParams m = ema_params(n);
    hipLaunchKernelGGL(k_ema_lerp, dim3(grid1d(n->n_pad / 4, 256)), dim3(256), 0, n->stream, m.e, m.p0, m.a, n->n_pad);
    XTRY(n, hipGetLastError());
    return 0;
}

int rcn_hipx_set_ema(rcn_hipx_net* n, float decay) {
    if (!n) return -1;
    if (!(std::isfinite(decay) && decay >= 0.f && decay < 1.f)) return fail(n, -1, "set_ema: decay must be finite and in [0, 1)");
    if (decay == n->ema_decay) return 0;
    Dev g(n->device);
    RTRY(reconfigure(n, {{decay != 0.f, &n->ema, padded_bytes(n), n->params.p}}));      // it starts as the live parameters
    n->ema_decay = decay;
    return 0;
}

int rcn_hipx_get_ema(const rcn_hipx_net* n, float* decay) {
    if (!n) return -1;
    if (decay) *decay = n->ema_decay;
    return 0;
}

int rcn_hipx_get_ema_params(rcn_hipx_net* n, float* flat) {
    if (!n || !flat) return -1;
    if (!n->ema.p) return fail(n, -6, "get_ema_params: the net has no average (rcn_hipx_set_ema with a decay > 0 first)");
    Dev g(n->device);
    return unpad(n, (const float*)n->ema.p, flat);
}

int rcn_hipx_set_ema_params(rcn_hipx_net* n, const float* flat) {
    if (!n || !flat) return -1;
    if (!n->ema.p) return fail(n, -6, "set_ema_params: the net has no average (rcn_hipx_set_ema with a decay > 0 first)");
    Dev g(n->device);
    return upload_padded(n, n->ema, flat);
}

int rcn_hipx_reset_ema(rcn_hipx_net* n) {
    if (!n) return -1;
    if (!n->ema.p) return 0;
    Dev g(n->device);
    XTRY(n, hipMemcpyAsync(n->ema.p, n->params.p, padded_bytes(n), hipMemcpyDeviceToDevice, n->stream));
    return 0;
}

int rcn_hipx_apply_sgd_dev(rcn_hipx_net* n, const float* grad, float grad_scale, float lr) {
    if (!n || !grad) return -1;
    Dev g(n->device);
    if (adam_on(*n)) {
        // Adam: the tick, then k_adam_apply; clipping on: the norm of fl(grad_scale * g) in front, the coefficient in front of the update
        if ((uintptr_t)grad % 16 != 0) return fail(n, -1, "apply_sgd: the gradient buffer must be 16-byte aligned");
        const bool clip = clip_on(*n);
        if (clip) {
            launch_sumsq(n, grad, n->n_pad, grad_scale, (double*)n->clip_part.p);
            XTRY(n, hipGetLastError());
        }
        launch_adam_tick(n);
        XTRY(n, hipGetLastError());
        const dim3 grid(grid1d(n->n_pad / 4, kClipThreads)), block(kClipThreads);
        if (clip) hipLaunchKernelGGL(k_adam_apply<true>, grid, block, 0, n->stream, (float*)n->params.p, grad, grad_scale, lr, adam_params(n), n->n_pad, clip_params(n));
        else hipLaunchKernelGGL(k_adam_apply<false>, grid, block, 0, n->stream, (float*)n->params.p, grad, grad_scale, lr, adam_params(n), n->n_pad, ClipParams{});
        XTRY(n, hipGetLastError());
    } else if (clip_on(*n)) {
        // clipping on, whatever the optimiser: the norm of fl(grad_scale * g), then k_sgd_apply with the coefficient in front of the update
        if ((uintptr_t)grad % 16 != 0) return fail(n, -1, "apply_sgd: the gradient buffer must be 16-byte aligned");
        launch_sumsq(n, grad, n->n_pad, grad_scale, (double*)n->clip_part.p);
        XTRY(n, hipGetLastError());
        const dim3 grid(grid1d(n->n_pad / 4, kClipThreads)), block(kClipThreads);
        if (sgd_default(*n)) hipLaunchKernelGGL(k_sgd_apply_clip<true>, grid, block, 0, n->stream, (float*)n->params.p, grad, grad_scale, lr, sgd_params(n), n->n_pad, clip_params(n));
        else hipLaunchKernelGGL(k_sgd_apply_clip<false>, grid, block, 0, n->stream, (float*)n->params.p, grad, grad_scale, lr, sgd_params(n), n->n_pad, clip_params(n));
        XTRY(n, hipGetLastError());
    } else if (sgd_default(*n)) RTRY(launch_axpy(n, grad, grad_scale * lr));      // plain SGD: rcn_hipx_apply_dev(grad, grad_scale * lr)'s launch
    else {
        if ((uintptr_t)grad % 16 != 0) return fail(n, -1, "apply_sgd: the gradient buffer must be 16-byte aligned");
        hipLaunchKernelGGL(k_sgd_apply, dim3(grid1d(n->n_pad / 4, 256)), dim3(256), 0, n->stream, (float*)n->params.p, grad, grad_scale, lr, sgd_params(n), n->n_pad);
        XTRY(n, hipGetLastError());
    }
    RTRY(apply_ema(n));
    return refresh_flipped(n);
}

int rcn_hipx_set_clip(rcn_hipx_net* n, float max_norm) {
    if (!n) return -1;
    if (!(max_norm >= 0.f)) return fail(n, -1, "set_clip: max_norm must be 0 (off) or > 0 (+inf: measure only)");
    if (max_norm == 0.f) max_norm = 0.f;                // (-0)
    if (max_norm == n->clip_max) return 0;
    Dev g(n->device);
    const bool on = max_norm != 0.f;
    RTRY(reconfigure(n, {{on, &n->clip_grad, padded_bytes(n), nullptr}, {on, &n->clip_part, (size_t)clip_blocks(n->n_pad) * sizeof(double), nullptr},
                         {on, &n->clip_state, sizeof(unsigned long long) + 2 * sizeof(float), nullptr}}));
    n->clip_max = max_norm;
    return 0;
}

int rcn_hipx_get_clip(const rcn_hipx_net* n, float* max_norm) {
    if (!n) return -1;
    if (max_norm) *max_norm = n->clip_max;
    return 0;
}

int rcn_hipx_set_accumulate(rcn_hipx_net* n, int k) {
    if (!n) return -1;
    if (k < 1 || k > 65536) return fail(n, -1, "set_accumulate: k must be in 1 .. 65536");
    if (k == n->accum_k) return 0;
    Dev g(n->device);
    // The accumulator is zeroed although a cycle's first micro-step stores: k_grad_sumsq and rcn_hipx_get_accumulated read all n_pad floats,
    // so any element outside the reduction jobs' [W | b] ranges has to be zero, and a read before the first micro-step has to be defined.
    RTRY(reconfigure(n, {{k > 1, &n->accum, padded_bytes(n), nullptr}}));
    n->accum_k = k; n->accum_c = 1.0f / (float)k; n->accum_pos = 0;      // (a pending cycle is discarded: the next micro-step is a first one and stores)
    return 0;
}

int rcn_hipx_get_accumulate(const rcn_hipx_net* n, int* k, int* pending) {
    if (!n) return -1;
    if (k) *k = n->accum_k;
    if (pending) *pending = n->accum_pos;
    return 0;
}

int rcn_hipx_reset_accumulation(rcn_hipx_net* n) {
    if (!n) return -1;
    n->accum_pos = 0;                                   // host state only: the next micro-step is a first one and stores
    return 0;
}

int rcn_hipx_get_accumulated(rcn_hipx_net* n, float* flat) {
    if (!n || !flat) return -1;
    if (!n->accum.p) return fail(n, -6, "get_accumulated: accumulation was never switched on (rcn_hipx_set_accumulate with k > 1 first)");
    Dev g(n->device);
    return unpad(n, (const float*)n->accum.p, flat);
}

int rcn_hipx_get_grad_norm(rcn_hipx_net* n, float* norm, float* coef) {
    if (!n) return -1;
    if (!n->clip_state.p) return fail(n, -6, "get_grad_norm: clipping was never switched on (rcn_hipx_set_clip with a max_norm > 0 first)");
    Dev g(n->device);
    float pair[2] = {0.f, 0.f};
    XTRY(n, hipMemcpyAsync(pair, (const char*)n->clip_state.p + sizeof(unsigned long long), sizeof pair, hipMemcpyDeviceToHost, n->stream));
    XTRY(n, hipStreamSynchronize(n->stream));
    if (norm) *norm = pair[0];
    if (coef) *coef = pair[1];
    return 0;
}

int rcn_hipx_set_grad_norm_log(rcn_hipx_net* n, float* log_dev, int64_t cap) {
    if (!n) return -1;
    if (log_dev && cap < 1) return fail(n, -1, "set_grad_norm_log: a log needs cap >= 1");
    Dev g(n->device);
    // the counter restarts, behind whatever the stream still holds (none yet: it starts at zero when rcn_hipx_set_clip makes it)
    if (n->clip_state.p) XTRY(n, hipMemsetAsync(n->clip_state.p, 0, sizeof(unsigned long long), n->stream));
    RTRY(reconfigure(n));                               // (the pointer is a kernel argument)
    n->clip_log = log_dev; n->clip_log_cap = log_dev ? (long long)cap : 0;
    return 0;
}

int rcn_hipx_get_grad_norm_count(rcn_hipx_net* n, int64_t* count) {
    if (!n || !count) return -1;
    Dev g(n->device);
    unsigned long long c = 0;
    if (n->clip_state.p) XTRY(n, hipMemcpyAsync(&c, n->clip_state.p, sizeof c, hipMemcpyDeviceToHost, n->stream));
    XTRY(n, hipStreamSynchronize(n->stream));
    *count = (int64_t)c;
    return 0;
}

int rcn_hipx_grad_norm_dev(rcn_hipx_net* n, const float* g_dev, int64_t len, float scale, float* norm_dev) {
    if (!n) return -1;
    if (!norm_dev || len < 0 || len % 4 != 0 || (len > 0 && (!g_dev || (uintptr_t)g_dev % 16 != 0)))
        return fail(n, -1, "grad_norm: n >= 0, n % 4 == 0, a 16-byte aligned buffer and a device float for the norm");
    Dev g(n->device);
    const long long nblk = clip_blocks((long long)len);
    if (nblk > 0x7fffffffLL) return fail(n, -1, "grad_norm: more than 2^43 elements");
    XTRY(n, n->norm_part.ensure((size_t)(nblk > 0 ? nblk : 1) * sizeof(double)));
    launch_sumsq(n, g_dev, (long long)len, scale, (double*)n->norm_part.p);
    XTRY(n, hipGetLastError());
    hipLaunchKernelGGL(k_grad_norm_finish, dim3(1), dim3(kClipThreads), 0, n->stream, (const double*)n->norm_part.p, (int)nblk, norm_dev);
    XTRY(n, hipGetLastError());
    return 0;
}

}  // extern "C"
