"""Track X's save and resume on the GPU (include/rcn_hipx.h: rcn_hipx_snapshot_dev / rcn_hipx_restore_dev; ConvNet.snapshot, save, load,
load_state): the pack launch against the getters; a snapshot as a point on the stream that disturbs nothing; a run stopped inside an
accumulation cycle, saved, closed and resumed in a net that was never configured by hand, bit-identical to the unbroken run; a restore
into a dirty net; a parameters-only snapshot; and the refusals, each of which leaves the net bit for bit what it was.  Every comparison
is of bit patterns: the feature is a copy."""
import ctypes as C

import numpy as np
import pytest
from _convnet_util import FUSED_HEAD, KW, MOMENTUM, NESTEROV, ODD_WIDTH, PLAIN_HEAD, batches, bits, dev, epoch, same_bits, sync, twins

pytestmark = pytest.mark.gpu

ADAMW = dict(betas=(0.9, 0.99), eps=1e-8, weight_decay=0.01, decoupled=True)
LR = 0.05


def has_site(spec):
    return any(l[0] == "dense_relu" for l in spec[1])


def configure(net, spec, opt="adamw", k=3):
    """AdamW (or an SGD triple), EMA, clip 1.0, accumulate k, and dropout 0.5 where the net has a dense_relu layer"""
    if opt == "adamw":
        net.set_adam(**ADAMW)
    else:
        net.set_sgd(*opt)
    net.set_ema(0.99)
    net.set_clip(1.0)
    net.set_accumulate(k)
    if has_site(spec):
        net.set_dropout(0.5, 11)


def micro_steps(net, data, lr=LR):
    """the batches of `data` as training steps, enqueued back to back with no synchronise in between"""
    import torch
    with torch.cuda.stream(net.stream):
        for x, y in data:
            net.train_step(x, y, lr)


def _or_none(f):
    from mercer_research_amd.convnet import ConvNetError
    try:
        return f()
    except ConvNetError:
        return None


def full_state(net):
    """everything the getters return, as bytes and numbers that compare with =="""
    adam = _or_none(net.get_adam_state)
    ema, acc = _or_none(net.get_ema), _or_none(net.get_accumulated)
    for a in (net.get_params(), net.get_velocity(), ema, acc) + (adam[:2] if adam else ()):
        assert a is None or not np.isnan(a).any()
    norm = _or_none(net.grad_norm)
    return {"params": net.get_params().tobytes(), "velocity": net.get_velocity().tobytes(),
            "adam_m": adam[0].tobytes() if adam else None, "adam_v": adam[1].tobytes() if adam else None, "adam_step": adam[2] if adam else None,
            "ema": ema.tobytes() if ema is not None else None, "accum": acc.tobytes() if acc is not None else None,
            "accumulate": net.get_accumulate(), "dropout_state": net.dropout_state(),
            "grad_norm": tuple(np.float32(v).tobytes() for v in norm) if norm else None, "grad_norm_count": net.grad_norm_count()}


def settings(net):
    return {"sgd": net.get_sgd(), "adam": net.get_adam(), "loss": net.get_loss(), "ema": net.get_ema_decay(), "clip": net.get_clip(),
            "accumulate": net.get_accumulate()[0], "dropout": net.get_dropout()}


def logits(net, x):
    """forward on the net's stream, read once that stream has got there"""
    import torch
    with torch.cuda.stream(net.stream):
        out = net.forward(x)
    net.synchronize()
    return out.cpu().numpy()


def differing(a, b):
    return sorted(k for k in a if a[k] != b[k])


# ---- 1. the pack launch against the getters -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("spec", [FUSED_HEAD, PLAIN_HEAD, ODD_WIDTH], ids=["fused_head", "plain_head", "odd_width"])
@pytest.mark.parametrize("opt", ["adamw", MOMENTUM], ids=["adamw", "momentum"])
def test_pack_equals_the_getters(spec, opt):
    from mercer_research_amd.convnet import SECTIONS, STATE_HAS
    net, = twins(spec, "fp32", 1)
    configure(net, spec, opt)
    micro_steps(net, batches(net, spec, 4))
    snap = net.snapshot()
    d, body = snap.desc, snap.body_bytes()
    net.synchronize()
    want = ["params", "ema", "accum"] + (["adam_m", "adam_v"] if opt == "adamw" else ["velocity"])
    assert d.sections == sum(SECTIONS[s] for s in want) and d.body_bytes == body.size
    assert d.n_log == net.n_logical and d.shape_and_layers() == (spec[0], [tuple(l) for l in spec[1]])
    assert same_bits(d.section(body, "params"), net.get_params())
    assert same_bits(d.section(body, "ema"), net.get_ema())
    assert same_bits(d.section(body, "accum"), net.get_accumulated()) and np.any(d.section(body, "accum") != 0)
    sc = d.scalars(body)
    if opt == "adamw":
        m, v, step = net.get_adam_state()
        assert same_bits(d.section(body, "adam_m"), m) and same_bits(d.section(body, "adam_v"), v) and np.any(v != 0)
        assert sc["adam_step"] == step == 1 and d.optim == 1
    else:
        assert same_bits(d.section(body, "velocity"), net.get_velocity()) and np.any(net.get_velocity() != 0)
        assert sc["adam_step"] is None and d.optim == 0 and not d.flags & STATE_HAS["adam_tick"]
    assert sc["dropout_state"] == (net.dropout_state() if has_site(spec) else None) and sc["dropout_state"] in (4, None)
    norm, coef = net.grad_norm()
    assert np.float32(sc["grad_norm"]).tobytes() == np.float32(norm).tobytes() and np.float32(sc["clip_coef"]).tobytes() == np.float32(coef).tobytes()
    assert sc["clip_count"] == net.grad_norm_count() == 1
    assert (d.accum_k, d.accum_pos) == net.get_accumulate() == (3, 1)
    assert not body[56:256].any()                       # the rest of the scalars block
    net.close()


# ---- 2. a point on the stream that disturbs nothing -----------------------------------------------------------------------------------------
def test_snapshot_is_a_point_on_the_stream_and_disturbs_nothing():
    spec = FUSED_HEAD
    a, b, c = twins(spec, "fp32", 3)
    for n in (a, b, c):
        configure(n, spec, "adamw", k=2)
    data = batches(a, spec, 5)
    # every graph exists before the comparison starts (a first use runs eagerly and captures), on all three alike: six micro-steps, so each
    # batch has been seen as the kind of micro-step it is below and the cycle is closed again
    for n in (a, b, c):
        micro_steps(n, data + data[:1])
        n.synchronize()
    g0, plan0 = a.graphs_instantiated(), a.plan_of_this_net(spec[2])
    import torch
    with torch.cuda.stream(a.stream):
        for x, y in data[:3]:
            a.train_step(x, y, LR)
        snap = a.snapshot()                             # no synchronise in front of it ...
        assert a.graphs_instantiated() == g0 and a.plan_of_this_net(spec[2]) == plan0
        for x, y in data[3:]:
            a.train_step(x, y, LR)                      # ... and none behind it
    micro_steps(b, data)
    micro_steps(c, data[:3])
    for n in (a, b, c):
        n.synchronize()
    ref = c.snapshot()
    assert bytes(snap.desc) == bytes(ref.desc)
    assert snap.body_bytes().tobytes() == ref.body_bytes().tobytes()
    assert differing(full_state(a), full_state(b)) == []
    assert a.graphs_instantiated() == b.graphs_instantiated() == g0
    assert a.plan_of_this_net(spec[2]) == plan0 == b.plan_of_this_net(spec[2])
    for n in (a, b, c):
        n.close()


# ---- 3. resume is bit-identical -------------------------------------------------------------------------------------------------------------
ROWS, NB = 40, 8


def resume(path, opt, precision, tamper=None):
    """(state, settings, losses 4..7) of the unbroken run A and of the run B -> file -> C; tamper(desc): changes the file's descriptor on
    its way (the by-hand check that each carried piece is needed)."""
    import torch
    from mercer_research_amd.convnet import Augment, ConvNet, mix_plan, read_state_file, warmup_cosine, write_state_file
    spec = FUSED_HEAD
    (H, W, _), _, B = spec
    a, b = twins(spec, precision, 2)
    for n in (a, b):
        configure(n, spec, opt)
        n.set_loss(0.1)
    rng = np.random.default_rng(3)
    X = dev(a, rng.integers(0, 256, (ROWS,) + spec[0]).astype(np.uint8))
    y = dev(a, rng.integers(0, 10, ROWS).astype(np.int32))
    perm = dev(a, rng.permutation(ROWS).astype(np.int32))
    lr = dev(a, warmup_cosine(NB, 0.05, 2, 0.005))
    aug = Augment(pad=2, hflip=True, seed=3, epoch=1)
    rec = mix_plan(NB, H, W, mixup_alpha=0.8, cutmix_alpha=1.0, seed=5)
    for s in (0, 5):
        rec[s] = (0.4, 0.4, 0, 0, 0, 0)                 # whatever the draws are: both kinds in both halves
    for s in (1, 4):
        rec[s] = (1.0, np.float32(1.0 - 6.0 / (H * W)), 1, 3, 2, 5)
    recs = a.mix_to_device(rec)
    la, lc = torch.zeros(NB, dtype=torch.float32, device=a.device), torch.zeros(NB // 2, dtype=torch.float32, device=a.device)
    sync()
    epoch(a, X, y, perm, B, lr, losses=la, augment=aug, mix=recs, **KW)
    epoch(b, X, y, perm, B, lr[:4].contiguous(), n_batches=4, augment=aug, mix=recs[:4].contiguous(), **KW)
    assert b.get_accumulate() == (3, 1)                 # stopped inside a cycle
    b.save(path, extra=b"next batch 4")
    b.close()
    if tamper is not None:
        desc, body, extra = read_state_file(open(path, "rb").read())
        tamper(desc)
        open(path, "wb").write(write_state_file(desc, body, extra))
    c, extra = ConvNet.load(path, max_batch=B)
    assert extra == b"next batch 4"
    epoch(c, X, y, perm, B, lr[4:].contiguous(), first_batch=4, n_batches=4, losses=lc, augment=aug, mix=recs[4:].contiguous(), **KW)
    out = ((full_state(a), settings(a), la.cpu().numpy()[4:].tobytes()), (full_state(c), settings(c), lc.cpu().numpy().tobytes()))
    a.close(); c.close()
    return out


@pytest.mark.parametrize("opt,precision", [("adamw", "fp32"), (NESTEROV, "fp32"), ("adamw", "bf16")], ids=["adamw", "nesterov", "adamw_bf16"])
def test_resume_is_bit_identical(tmp_path, opt, precision):
    (sa, ga, la), (sc, gc, lc) = resume(str(tmp_path / "run.rcnx"), opt, precision)
    assert differing(sa, sc) == []
    assert ga == gc
    assert la == lc and len(set(np.frombuffer(la, dtype=np.float32).tolist())) == 4
    assert sa["accumulate"] == (3, 2) and sa["dropout_state"] == NB and sa["grad_norm_count"] == 2
    assert sa["adam_step"] == (2 if opt == "adamw" else None)


# ---- 4. restore into a dirty net ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("spec", [FUSED_HEAD, PLAIN_HEAD], ids=["fused_head", "plain_head"])
def test_restore_into_a_dirty_net(spec):
    import torch
    src, = twins(spec, "fp32", 1, seed=1)
    dst, = twins(spec, "fp32", 1, seed=9)
    configure(src, spec, "adamw")
    src.set_loss(0.1)
    micro_steps(src, batches(src, spec, 4, seed=0))
    # the target: other parameters, another recipe, other data, and padding that is not zero
    dst.set_adam(betas=(0.8, 0.9), eps=1e-6, weight_decay=0.0, decoupled=False)
    dst.set_ema(0.5); dst.set_clip(5.0); dst.set_accumulate(2); dst.set_loss(0.2)
    if has_site(spec):
        dst.set_dropout(0.25, 3)
    micro_steps(dst, batches(dst, spec, 3, seed=50), lr=0.1)
    with torch.cuda.stream(dst.stream):
        dst.apply(torch.ones(dst.n_padded, dtype=torch.float32, device=dst.device), 0.25)      # every element, padding included
    dst.synchronize()
    assert differing(full_state(src), full_state(dst)) != [] and settings(src) != settings(dst)
    snap = src.snapshot()
    assert dst.load_state(snap) is None
    assert differing(full_state(src), full_state(dst)) == []
    assert settings(src) == settings(dst)
    again = dst.snapshot()
    assert bytes(again.desc) == bytes(snap.desc) and again.body_bytes().tobytes() == snap.body_bytes().tobytes()
    # one more identical step on both: the cycle closes (position 1 -> 2 of 3) ... and one more, so an update runs on both
    more = batches(src, spec, 2, seed=70)
    micro_steps(src, more)
    micro_steps(dst, more)
    fs, fd = full_state(src), full_state(dst)
    assert differing(fs, fd) == [] and fs["accumulate"] == (3, 0) and fs["adam_step"] == 2
    src.close(); dst.close()


# ---- 5. the parameters alone ----------------------------------------------------------------------------------------------------------------
def test_model_only(tmp_path):
    from mercer_research_amd.convnet import SECTIONS, ConvNet
    spec = FUSED_HEAD
    src, = twins(spec, "fp32", 1)
    plain, = twins(spec, "fp32", 1)                       # never configured: what "the default recipe" reads as
    configure(src, spec, "adamw")
    data = batches(src, spec, 4)
    micro_steps(src, data)
    snap = src.snapshot("model")
    n_log = src.n_logical
    assert snap.desc.sections == SECTIONS["params"] and snap.desc.flags == 0
    assert snap.desc.body_bytes == 256 + (4 * n_log + 255) // 256 * 256 == snap.body_bytes().size
    path = str(tmp_path / "model.rcnx")
    snap.save(path)
    got, extra = ConvNet.load(path, max_batch=spec[2])
    assert extra is None
    assert settings(got) == settings(plain)
    fg = full_state(got)
    assert fg["adam_m"] is None and fg["ema"] is None and fg["accum"] is None and fg["dropout_state"] == 0
    assert same_bits(got.get_params(), src.get_params())
    x = data[0][0]
    assert same_bits(logits(got, x), logits(src, x))
    # into a configured net: its recipe and optimiser state stay as they are
    keep, = twins(spec, "fp32", 1, seed=4)
    configure(keep, spec, "adamw")
    micro_steps(keep, data[:3])
    before, s0 = full_state(keep), settings(keep)
    keep.load_state(snap)
    assert differing(before, full_state(keep)) == ["params"] and settings(keep) == s0
    assert same_bits(keep.get_params(), src.get_params())
    for n in (src, plain, got, keep):
        n.close()


# ---- 6. refusals leave the net alone --------------------------------------------------------------------------------------------------------
def test_refusals_leave_the_net_alone():
    import torch
    from mercer_research_amd.convnet import SECTIONS, StateDesc
    spec = FUSED_HEAD
    net, twin = twins(spec, "fp32", 2)
    for n in (net, twin):
        configure(n, spec, "adamw")
    data = batches(net, spec, 5)
    for n in (net, twin):
        micro_steps(n, data[:4])
        n.synchronize()
    snap = net.snapshot()
    body, nbytes = snap.body, int(snap.desc.body_bytes)
    micro_steps(net, data[4:])                          # the net moves on: a restore that went through would show
    micro_steps(twin, data[4:])
    net.synchronize()
    state0, set0, g0 = full_state(net), settings(net), net.graphs_instantiated()
    lib, h = net.lib, net.net

    def changed(**fields):
        d = StateDesc.from_buffer_copy(bytes(snap.desc))
        for k, v in fields.items():
            setattr(d, k, v)
        return d

    other_layers = changed()
    other_layers.layers[2].out = 32
    ptr = C.c_void_p(body.data_ptr())
    cases = [("layer list", other_layers, ptr, nbytes, -2), ("input shape", changed(in_h=spec[0][0] + 2), ptr, nbytes, -2),
             ("body_bytes too small", snap.desc, ptr, nbytes - 1, -1), ("version", changed(version=snap.desc.version + 1), ptr, nbytes, -1),
             ("magic", changed(magic=0), ptr, nbytes, -1), ("misaligned body", snap.desc, C.c_void_p(body.data_ptr() + 4), nbytes, -1),
             ("section outside the body", changed(body_bytes=nbytes - 256), ptr, nbytes, -1), ("accum_pos out of range", changed(accum_pos=3), ptr, nbytes, -1)]
    for name, d, p, nb, want in cases:
        assert lib.rcn_hipx_restore_dev(h, C.byref(d), p, nb) == want, name
        assert differing(state0, full_state(net)) == [] and settings(net) == set0 and net.graphs_instantiated() == g0, name
    # snapshots that are refused: too little room, a misaligned body, a section the net does not have
    out = StateDesc()
    assert lib.rcn_hipx_snapshot_dev(h, 0, ptr, nbytes - 1, C.byref(out)) == -1
    assert lib.rcn_hipx_snapshot_dev(h, 0, C.c_void_p(body.data_ptr() + 4), nbytes, C.byref(out)) == -1
    assert lib.rcn_hipx_snapshot_dev(h, SECTIONS["velocity"], ptr, nbytes, C.byref(out)) == -6
    assert lib.rcn_hipx_snapshot_dev(h, 0, None, nbytes, C.byref(out)) == -1 and lib.rcn_hipx_snapshot_dev(h, 0, ptr, nbytes, None) == -1
    # between rcn_hipx_gradients_begin_dev and the last bucket
    seen = {}

    def on_bucket(_, k, n):
        if k == 0:
            seen["n"] = n
            seen["restore"] = lib.rcn_hipx_restore_dev(h, C.byref(snap.desc), ptr, nbytes)
            seen["snapshot"] = lib.rcn_hipx_snapshot_dev(h, 0, ptr, nbytes, C.byref(out))
    x, y = data[0]
    for n in (net, twin):                               # (a gradient walk is a training forward: the twin counts it too)
        with torch.cuda.stream(n.stream):
            grad = torch.empty(n.n_padded, dtype=torch.float32, device=n.device)
            n.gradients_bucketed(x, y, grad, min_bucket_bytes=0, on_bucket=on_bucket if n is net else None)
        n.synchronize()
    assert seen["n"] > 1 and seen["restore"] == -6 and seen["snapshot"] == -6
    state0["dropout_state"] += 1
    assert differing(state0, full_state(net)) == [] and settings(net) == set0
    # the next step is the twin's
    more = batches(net, spec, 2, seed=90)
    micro_steps(net, more)
    micro_steps(twin, more)
    assert differing(full_state(net), full_state(twin)) == []
    # and the walk over, both calls go through again
    assert lib.rcn_hipx_snapshot_dev(h, 0, ptr, nbytes, C.byref(out)) == 0
    net.synchronize()
    net.close(); twin.close()


# ---- 7. the accumulator's setter ------------------------------------------------------------------------------------------------------------
def test_set_accumulated():
    from mercer_research_amd.convnet import ConvNetError
    spec = PLAIN_HEAD
    a, b = twins(spec, "fp32", 2, sgd=MOMENTUM)
    with pytest.raises(ConvNetError, match="-6"):
        b.set_accumulated(np.zeros(b.n_logical, dtype=np.float32), 0)
    for n in (a, b):
        n.set_accumulate(3)
    data = batches(a, spec, 3)
    micro_steps(a, data[:2])
    a.synchronize()
    for bad in (-1, 3):
        with pytest.raises(ConvNetError, match="-1"):
            b.set_accumulated(a.get_accumulated(), bad)
    assert b.get_accumulate() == (3, 0)
    b.set_accumulated(a.get_accumulated(), 2)
    assert b.get_accumulate() == (3, 2) and same_bits(a.get_accumulated(), b.get_accumulated())
    micro_steps(a, data[2:])
    micro_steps(b, data[2:])                            # the last micro-step of the cycle on both: the same update
    assert differing(full_state(a), full_state(b)) == [] and np.any(bits(a.get_velocity()) != 0)
    a.close(); b.close()
