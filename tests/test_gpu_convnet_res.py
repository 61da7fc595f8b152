"""GPU tests of Track X's residual blocks (include/rcn_hipx.h: RCN_HIPX_BN_ADD_RELU; csrc/convnet_bn.hpp: k_bn_apply_relu<EVAL, ADD>,
k_skip_bwd_add) against PyTorch on the CPU in float64 (tests/_torch_ref.py) on the four nets of tests/test_convnet_res_plan.py: the logits
of a training forward, the loss, the gradients per tensor, the running statistics, parameters and losses after plain SGD steps and the
forward / evaluation on the running statistics; the identity block (equal bits with the net without it), the gate of the skip's source,
and the skip inside the training recipe.

Tolerances are those of tests/test_gpu_convnet_bn.py: fp32 against f64 2e-4 of a tensor's scale + 1e-6, 4e-4 after
a second step; bf16 operands 5e-3 / 2e-2 against the twin with the SAME operand rounding, the training logits also 3e-2 against the
unrounded twin."""
import numpy as np
import pytest
from _convnet_util import LR, batches, close, dev, epoch, make_net, plan_lines, same_bits, step, twins
from _torch_ref import TorchNet, close_per_tensor, plain, random_params, tensor_slices
from _twin_checks import against_torch
from test_convnet_res_plan import RES_A, RES_B, RES_C, RES_NETS

pytestmark = pytest.mark.gpu

RTOL = {"fp32": 2e-4, "bf16": 5e-3}
RTOL_2 = {"fp32": 4e-4, "bf16": 2e-2}                   # after a second step
CASES = [("a", "fp32"), ("a", "bf16"), ("b", "fp32"), ("c", "fp32"), ("d", "fp32")]


def _data(spec, seed=3):
    in_shape, layers, B = spec
    rng = np.random.default_rng(seed)
    flat = random_params(rng, in_shape, layers)
    x = rng.standard_normal((B,) + in_shape).astype(np.float32)
    y = rng.integers(0, layers[-1][1], B).astype(np.int32)
    return flat, x, y


def _grads(net, xd, yd, B):
    """(logical gradient, loss, training logits) of one gradients call"""
    import torch
    loss = torch.zeros(1, dtype=torch.float32, device=net.device)
    with torch.cuda.stream(net.stream):
        g = net.gradients(xd, yd, loss=loss)
        z = net.last_logits(B)
    net.synchronize()
    return net.unpad(g), float(loss.item()), z.cpu().numpy()


def _run(spec, precision, flat, x, y, steps):
    """What the device and the float64 twin make of: one gradients call (a training forward: the statistics advance), `steps` plain SGD
    steps, then a forward and an evaluation on the running statistics."""
    import torch
    in_shape, layers, B = spec
    net = make_net(spec, precision)
    ref = TorchNet(in_shape, layers, flat, operand="bf16" if precision == "bf16" else "f64")
    net.set_params(flat)
    xd, yd = dev(net, x), dev(net, y)
    out = {}
    out["grad"], out["loss"], out["logits"] = _grads(net, xd, yd, B)
    out["stats1"] = net.get_bn_stats()
    out["ref_loss"], out["ref_logits"], out["ref_grad"] = ref.loss_and_grads(x, y)
    out["ref_stats1"] = ref.bn_stats().copy()
    loss = torch.zeros(1, dtype=torch.float32, device=net.device)
    losses = []
    for _ in range(steps):
        step(net, xd, yd, LR, loss)
        losses.append(float(loss.item()))
    out["losses"], out["ref_losses"] = losses, [ref.sgd_step(x, y, LR) for _ in range(steps)]
    out["params"], out["stats"], out["ref_params"], out["ref_stats"] = net.get_params(), net.get_bn_stats(), ref.params(), ref.bn_stats().copy()
    with torch.cuda.stream(net.stream):
        ze = net.forward(xd)
    net.synchronize()
    out["eval_logits"], out["ref_eval_logits"] = ze.cpu().numpy(), ref.logits(x, train=False)
    out["eval"] = net.evaluate(xd, yd, x_scale=1.0, x_shift=0.0)
    zr = out["ref_eval_logits"]
    lse = np.log(np.exp(zr - zr.max(1, keepdims=True)).sum(1)) + zr.max(1)
    out["ref_eval"] = (float((lse - zr[np.arange(B), y]).mean()), int((zr.argmax(1) == y).sum()))
    out["margin"] = float(np.min(np.sort(zr, axis=1)[:, -1] - np.sort(zr, axis=1)[:, -2]))
    net.close()
    return out


@pytest.fixture(scope="module", params=CASES, ids=[f"{n}-{p}" for n, p in CASES])
def case(request):
    name, precision = request.param
    spec = RES_NETS[name]
    steps = 1 if name == "d" else 2                       # (three float64 passes over net d's 133120 rows are the seconds this file may take)
    return name, precision, spec, steps, _run(spec, precision, *_data(spec), steps=steps)


def test_training_forward_logits_and_loss(case):
    name, precision, spec, _, r = case
    close(r["logits"], r["ref_logits"], RTOL[precision], f"{name} {precision} training logits")
    close([r["loss"]], [r["ref_loss"]], RTOL[precision], f"{name} {precision} loss")
    if precision == "bf16":
        flat, x, y = _data(spec)
        close(r["logits"], TorchNet(spec[0], spec[1], flat).logits(x, train=True), 3e-2, f"{name} bf16 training logits against the unrounded twin")


def test_gradients_per_tensor(case):
    name, precision, spec, _, r = case
    assert np.isfinite(r["grad"]).all()
    close_per_tensor(r["grad"], r["ref_grad"], spec[0], spec[1], RTOL[precision], f"{name} {precision} gradient")


def test_running_statistics_after_one_training_forward(case):
    name, precision, spec, _, r = case
    close(r["stats1"], r["ref_stats1"], RTOL[precision], f"{name} {precision} running statistics after gradients()")
    assert np.abs(r["stats1"] - r["stats"]).max() > 1e-3          # ... and they went on moving with the steps


def test_parameters_and_statistics_after_the_steps(case):
    name, precision, spec, steps, r = case
    rtol = (RTOL_2 if steps == 2 else RTOL)[precision]
    assert len(r["losses"]) == steps
    for got, ref in zip(r["losses"], r["ref_losses"]):
        close([got], [ref], rtol, f"{name} {precision} step loss")
    close_per_tensor(r["params"], r["ref_params"], spec[0], spec[1], rtol, f"{name} {precision} parameters")
    close(r["stats"], r["ref_stats"], rtol, f"{name} {precision} running statistics after {steps} steps")


def test_forward_and_evaluate_use_the_running_statistics(case):
    name, precision, spec, _, r = case
    close(r["eval_logits"], r["ref_eval_logits"], RTOL_2[precision], f"{name} {precision} evaluation logits")
    assert np.abs(r["eval_logits"] - r["logits"]).max() > 10 * RTOL_2[precision] * np.abs(r["ref_eval_logits"]).max()
    (loss, correct), (rloss, rcorrect) = r["eval"], r["ref_eval"]
    close([loss], [rloss], RTOL_2[precision], f"{name} {precision} evaluation loss")
    scale = float(np.abs(r["ref_eval_logits"]).max())
    if r["margin"] > 4 * RTOL_2[precision] * scale:       # no row's two best logits are within reach of the tolerance: the count is exact
        assert correct == rcorrect, (correct, rcorrect)


def test_create_refuses_what_the_plan_refuses():
    """describe_layers is one function: rcn_hipx_create returns the plan's status and message"""
    from mercer_research_amd import convnet
    from test_convnet_res_plan import REFUSALS
    for layers, status, index, _ in REFUSALS:
        with pytest.raises(convnet.ConvNetError) as plan_err:
            convnet.plan((4, 4, 32), layers, 2)
        with pytest.raises(convnet.ConvNetError) as create_err:
            convnet.ConvNet((4, 4, 32), layers, 2)
        assert str(plan_err.value) == f"rcn_hipx_plan: {status}: " + str(create_err.value).split(f"rcn_hipx_create: {status}: ", 1)[1]
        assert f"layer {index} " in str(create_err.value)
    net = make_net(RES_A, "fp32")
    with pytest.raises(convnet.ConvNetError, match="status -3.*batch normalisation"):
        net.set_precision("bf16_stored")
    assert net.get_bn()[2] == 2 and net.get_bn_stats().size == 2 * 2 * 32
    net.close()


# ---- the identity block ---------------------------------------------------------------------------------------------------------------------

def test_block_with_zero_gamma_and_beta_is_the_identity_bit_for_bit():
    """The block's second batch normalisation with gamma = 0, beta = 0: y = max(0, fl(fl(fl(xh * 0) + 0) + s)) = s for the post-ReLU s, so
    net a and `conv 32, pool, dense 10` with the same other parameters have EQUAL BITS in training logits, loss and forward logits.  The main
    path's gradient is zero behind that layer (dx = gamma * ...), so the first convolution and the dense layer get the plain net's gradient
    through the skip alone: 2e-4 per tensor, and equal bits where the two plans name the same weight-gradient launch."""
    import torch
    from mercer_research_amd import convnet
    in_shape, layers, B = RES_A
    plain_spec = (in_shape, (("conv", 32), ("pool",), ("dense", 10)), B)
    flat, x, y = _data(RES_A, seed=5)
    sl = tensor_slices(in_shape, layers)                  # conv 0, conv 1, bn 2, conv 3, bn 4, dense
    flat[sl[4][0]] = 0.0
    flat[sl[4][1]] = 0.0
    flat_plain = np.concatenate([flat[sl[0][0]], flat[sl[0][1]], flat[sl[5][0]], flat[sl[5][1]]])
    got = []
    for spec, p in ((RES_A, flat), (plain_spec, flat_plain)):
        net = make_net(spec, "fp32")
        net.set_params(p)
        xd, yd = dev(net, x), dev(net, y)
        g, loss, z = _grads(net, xd, yd, B)
        with torch.cuda.stream(net.stream):
            ze = net.forward(xd)
        net.synchronize()
        got.append((g, np.float32(loss), z, ze.cpu().numpy()))
        net.close()
    (ga, la, za, zea), (gp, lp, zp, zep) = got
    assert same_bits(za, zp) and same_bits(np.array([la]), np.array([lp]))
    # (the forward on the running statistics: gamma = beta = 0 there too)
    assert same_bits(zea, zep)
    psl = tensor_slices(plain_spec[0], plain_spec[1])
    pa, pp = plan_lines(convnet.plan(*RES_A)), plan_lines(convnet.plan(*plain_spec))
    for tag, prefix, a_sl, p_sl in (("first convolution", "wgrad conv3x3 8x8x3->32", sl[0], psl[0]), ("dense", "wgrad dense", sl[5], psl[1])):
        for part, u, v in (("weights", a_sl[0], p_sl[0]), ("biases", a_sl[1], p_sl[1])):
            close(ga[u], gp[v], 2e-4, f"identity block: {tag} {part} gradient against the plain net's")
        la_, = [t for t in pa if t.startswith(prefix)]
        lp_, = [t for t in pp if t.startswith(prefix)]
        print(f"{tag}: '{la_}' / '{lp_}'")
        if la_ == lp_:
            assert same_bits(ga[a_sl[0]], gp[p_sl[0]]) and same_bits(ga[a_sl[1]], gp[p_sl[1]]), tag
    # the main path really is shut: the block's inner layers get no gradient but the second BN's beta and gamma
    assert not ga[sl[1][0]].any() and not ga[sl[3][0]].any() and not ga[sl[2][0]].any()
    assert ga[sl[4][1]].any()


# ---- the gate of the skip's source ----------------------------------------------------------------------------------------------------------

def test_the_source_gate_shows():
    """Net c: both sources (layer 1, a bn_relu; layer 5, a bn_add_relu) are gated by the convolution above them, and the skip's share must
    pass the same gate.  On this batch between 20 % and 80 % of each source's output is zero, and the twin's gradient WITHOUT the source gate
    on the skip path differs from the true one by more than 10 x the tolerance in some tensor: the comparison below tells the two apart."""
    in_shape, layers, B = RES_C
    flat, x, y = _data(RES_C, seed=13)
    ref = TorchNet(in_shape, layers, flat)
    _, _, g_true = ref.loss_and_grads(x, y)
    for s in (1, 5):
        zero = float((ref.outs[s].detach().numpy() == 0).mean())
        print(f"layer {s}: {zero:.2f} of the output is zero")
        assert 0.2 <= zero <= 0.8, (s, zero)
    _, _, g_loose = TorchNet(in_shape, layers, flat, gate_source=False).loss_and_grads(x, y)
    worst = 0.0
    for ws, bs in tensor_slices(in_shape, layers):
        for t in (ws, bs):
            worst = max(worst, float(np.abs(g_loose[t] - g_true[t]).max()) / (2e-4 * max(1e-3, float(np.abs(g_true[t]).max())) + 1e-6))
    print(f"no source gate: worst |d| / allowance = {worst:.1f}")
    assert worst > 10.0, worst
    net = make_net(RES_C, "fp32")
    net.set_params(flat)
    g, _, _ = _grads(net, dev(net, x), dev(net, y), B)
    net.close()
    close_per_tensor(g, g_true, in_shape, layers, 2e-4, "net c, gated sources: gradient")


# ---- the recipe -----------------------------------------------------------------------------------------------------------------------------

def _state(net):
    return net.get_params(), net.get_bn_stats(), net.get_velocity()


def _same(a, b):
    return all(same_bits(u, v) for u, v in zip(a, b))


def _close(*nets):
    for n in nets:
        n.close()


def test_twins_are_bit_identical():
    a, b = twins(RES_A, "fp32", 2, sgd=(0.9, 0.0, False))
    for x, y in batches(a, RES_A, 3):
        step(a, x, y, LR)
        step(b, x, y, LR)
    assert _same(_state(a), _state(b)) and a.get_velocity().any()
    _close(a, b)


def test_overlap_changes_no_bit():
    """net b: the weight gradients on the second stream read out[S] and dout[S + 1], never the dout[S] the add writes"""
    a, b = twins(RES_B, "fp32", 2)
    b.set_overlap(1)
    x, y = batches(a, RES_B, 1)[0]
    ga, la, za = _grads(a, x, y, RES_B[2])
    gb, lb, zb = _grads(b, x, y, RES_B[2])
    assert same_bits(ga, gb) and la == lb and same_bits(za, zb)
    for _ in range(2):
        step(a, x, y, LR)
        step(b, x, y, LR)
    assert _same(_state(a), _state(b))
    _close(a, b)


@pytest.mark.parametrize("min_bytes", [0, 40000])
def test_buckets_that_cut_inside_a_block_change_no_bit(min_bytes):
    """net c: at 0 bytes every layer is a bucket; at 40000 the 37 KB convolutions pair up with a neighbour -- either way buckets end inside
    the blocks, between the add (in the iteration of layer S + 1) and layer S"""
    import torch
    net, = twins(RES_C, "fp32", 1)
    x, y = batches(net, RES_C, 1)[0]
    g, _, _ = _grads(net, x, y, RES_C[2])
    gb = torch.zeros(net.n_padded, dtype=torch.float32, device=net.device)
    seen = []
    with torch.cuda.stream(net.stream):
        net.gradients_bucketed(x, y, gb, min_bucket_bytes=min_bytes, on_bucket=lambda *a: seen.append(a))
    net.synchronize()
    assert len(seen) > 2 and same_bits(net.unpad(gb), g)
    net.close()


def test_epoch_equals_steps_and_adds_no_graph():
    in_shape, layers, B = RES_A
    a, b = twins(RES_A, "fp32", 2)
    flat_bn = make_net((in_shape, plain(layers), B), "fp32")            # the bn_relu net of the same depth
    flat_bn.init_params(1)
    rng = np.random.default_rng(2)
    n = 3 * B
    X, y = rng.standard_normal((n,) + in_shape).astype(np.float32), rng.integers(0, 10, n).astype(np.int32)
    perm = rng.permutation(n).astype(np.int32)
    Xd, yd, pd = dev(a, X), dev(a, y), dev(a, perm)
    epoch(a, Xd, yd, pd, B, LR)
    epoch(flat_bn, Xd, yd, pd, B, LR)
    for s in range(3):
        rows = perm[s * B:(s + 1) * B]
        step(b, dev(b, X[rows]), dev(b, y[rows]), LR)
    assert _same(_state(a), _state(b))
    assert a.graphs_instantiated() == flat_bn.graphs_instantiated() == 1
    _close(a, b, flat_bn)


def _against_torch(configure, make_optim, micro=1, rtol=4e-4, tag=""):
    """ONE update of `micro` micro-batches on net a on the device and in float64 torch (tests/_twin_checks.py: against_torch)"""
    against_torch(RES_A, configure, make_optim, micro, rtol, tag)


def test_adamw_step_against_torch():
    """eps = 1e-4 for the reason tests/test_gpu_convnet_bn_recipe.py gives: a convolution's bias in front of batch normalisation has gradient
    zero in exact arithmetic, and Adam would turn fp32 rounding noise there into steps."""
    import torch
    lr, wd = 1e-2, 0.05
    _against_torch(lambda n: n.set_adam((0.9, 0.999), 1e-4, wd, True), lambda p: (torch.optim.AdamW(p, lr=lr, betas=(0.9, 0.999), eps=1e-4, weight_decay=wd), lr, None), tag="AdamW")


def test_clipped_step_against_torch():
    import torch
    _against_torch(lambda n: n.set_clip(0.25), lambda p: (torch.optim.SGD(p, lr=LR), LR, 0.25), tag="clip 0.25")


def test_accumulate_two_against_torch():
    import torch
    _against_torch(lambda n: n.set_accumulate(2), lambda p: (torch.optim.SGD(p, lr=LR), LR, None), micro=2, tag="accumulate 2")


def test_save_and_load_rebuild_the_block_and_continue_bit_for_bit(tmp_path):
    from mercer_research_amd.convnet import ConvNet
    a, = twins(RES_A, "fp32", 1, sgd=(0.9, 5e-4, True))
    bs = batches(a, RES_A, 4)
    for x, y in bs[:2]:
        step(a, x, y, LR)
    path = tmp_path / "res.state"
    a.save(path, extra=b"loop state")
    b, extra = ConvNet.load(path, RES_A[2])
    assert extra == b"loop state" and b.layers == [tuple(l) for l in RES_A[1]] and b.layers[4] == ("bn_add_relu", 4)
    assert _same(_state(a), _state(b))
    for x, y in bs[2:]:
        step(a, x, y, LR)
        step(b, x, y, LR)
    assert _same(_state(a), _state(b))
    _close(a, b)
