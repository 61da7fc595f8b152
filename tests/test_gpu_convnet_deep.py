"""GPU tests of nets with 17 to 32 layers with parameters (tests/test_convnet_deep_plan.py: the nets, what each reaches and every condition
the references must meet): the job tables of the reduction launch (k_reduce_all..., k_reduce_all_acc: ReduceJobs), of the state pack
(k_state_pack / k_state_unpack: StateJobs) and of the bf16 operand copies (k_prep_all_bf16: PrepJobs) past entry 15, and the per-launch
k_prep_weights_bf16 copies a net with more than 16 matrix layers behind layer 0 falls back to.

fp32: against PyTorch on the CPU in float64 (tests/_torch_ref.py) at the project's bound, 2e-4 of a tensor's scale + 1e-6
and 4e-4 after a second step -- but for the gradient of P32's conv_linear biases, exactly zero in the twin, whose allowance is 4 x what a
float32 CPU evaluation of the same net needs (tests/test_convnet_deep_plan.py: ZERO_BIAS_FACTOR).  bf16: the exact integer nets of P17 and
P18 against the oracle, logits bit for bit; P32 and RES20 device against device only -- the bf16-operand twin moves by 96 (P32) and 1.0
(RES20) of its own allowances under a 6e-8 perturbation and cannot judge the device there."""
import numpy as np
import pytest
from _convnet_util import LR, NESTEROV, batches, close_per_tensor, dev, epoch, make_net, same_bits, step, twins
from _ema_ref import ema_update
from _exact_nets import MODES
from _oracle_steps import LR as EXACT_LR
from _torch_ref import tensor_slices
from _twin_checks import against_torch, compare, device_run, grads, stats
from test_convnet_deep_plan import (DEEP_NETS, EXACT_NETS, P18, P32, P33, RTOL, RTOL_2, SEEDS, STEPS, ZERO_BIAS_FACTOR, _optimisers, adamw_widened, data,
                                    exact_case, exact_reference, twin_run, zero_bias_tensors)

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("name", sorted(DEEP_NETS))
def test_against_the_twin(name):
    spec = DEEP_NETS[name]
    r = device_run(spec, "fp32", *data(spec, SEEDS[name]), STEPS)
    widened = {t: ZERO_BIAS_FACTOR[name] for t in zero_bias_tensors(spec[1])} if ZERO_BIAS_FACTOR[name] != 1.0 else None
    compare(spec, r, twin_run(name), RTOL, RTOL_2, STEPS, f"{name} fp32", widened_gradients=widened)


# ---- one update of each family on P32 against float64 torch ------------------------------------------------------------------------------------

def _buffered(net, launches):
    """the update reads the step's gradient from a buffer as 32 one-chunk slabs: the second table of the reduction launch is full"""
    text = net.plan_of_this_net(P32[2])
    assert " 32 layers' gradients as one-chunk slabs" in text and all(k in text for k in launches), text


def _family(name, configure, widened=None):
    make_optim, micro = _optimisers()[name]
    against_torch(P32, configure, make_optim, micro, RTOL_2, f"P32 {name}", widened)


def test_nesterov_momentum_and_weight_decay_against_torch():
    _family("nesterov", lambda n: n.set_sgd(0.9, 5e-4, True))


def test_adamw_step_against_torch():
    """eps = 1e-4 for the reason tests/test_gpu_convnet_res.py gives.  The conv_linear layers' parameters at 4 x the float32 CPU
    evaluation's own distance from the twin (tests/test_convnet_deep_plan.py: ADAMW_FLOAT32_SHARE), everything else at 4e-4."""
    _family("adamw", lambda n: n.set_adam((0.9, 0.999), 1e-4, 0.05, True), adamw_widened())


def test_clipped_step_against_torch():
    def configure(n):
        n.set_clip(0.25)
        _buffered(n, ("k_grad_sumsq", "k_reduce_all_clip"))
    _family("clip", configure)


def test_accumulate_two_against_torch():
    def configure(n):
        n.set_accumulate(2)
        _buffered(n, ("k_reduce_all_acc<next>",))
        assert "k_reduce_all_acc<first>" in n.plan_micro_of_this_net(P32[2], "first")
    _family("accumulate", configure)


def test_ema_after_two_steps_is_the_host_formula():
    net, = twins(P32, "fp32", 1)
    net.set_ema(0.9)
    e = net.get_ema()
    assert same_bits(e, net.get_params())
    for x, y in batches(net, P32, 2):
        step(net, x, y, LR)
        e = ema_update(e, net.get_params(), 0.9)
    assert same_bits(net.get_ema(), e) and not same_bits(e, net.get_params())
    for li, (ws, _) in enumerate(tensor_slices(P32[0], P32[1])):          # every layer's average lags its weights
        assert np.abs(e[ws] - net.get_params()[ws]).max() > 0, li
    net.close()


def _state(net):
    return net.get_params(), stats(net), net.get_velocity()


def _same(a, b):
    return all(same_bits(u, v) for u, v in zip(a, b))


def _close(*nets):
    for n in nets:
        n.close()


def test_epoch_with_a_device_learning_rate_equals_three_steps_on_one_graph():
    in_shape, layers, B = P32
    a, b = twins(P32, "fp32", 2)
    rng = np.random.default_rng(2)
    n = 3 * B
    X, y = rng.standard_normal((n,) + in_shape).astype(np.float32), rng.integers(0, layers[-1][1], n).astype(np.int32)
    perm = rng.permutation(n).astype(np.int32)
    rates = np.array([0.05, 0.03, 0.01], dtype=np.float32)
    epoch(a, dev(a, X), dev(a, y), dev(a, perm), B, dev(a, rates))
    for s in range(3):
        rows = perm[s * B:(s + 1) * B]
        step(b, dev(b, X[rows]), dev(b, y[rows]), float(rates[s]))
    assert _same(_state(a), _state(b))
    assert a.graphs_instantiated() == 1
    _close(a, b)


@pytest.mark.parametrize("min_bytes", [0, 40000])
def test_buckets_change_no_bit(min_bytes):
    """at 0 bytes every layer with parameters is a bucket: 32 of them; at 40000 the 37 KB convolutions pair up with a batch normalisation"""
    import torch
    net, = twins(P32, "fp32", 1)
    x, y = batches(net, P32, 1)[0]
    g, _, _ = grads(net, x, y, P32[2])
    gb = torch.zeros(net.n_padded, dtype=torch.float32, device=net.device)
    seen = []
    with torch.cuda.stream(net.stream):
        net.gradients_bucketed(x, y, gb, min_bucket_bytes=min_bytes, on_bucket=lambda *a: seen.append(a))
    net.synchronize()
    assert (len(seen) == 32) if min_bytes == 0 else (2 < len(seen) < 32), len(seen)
    assert same_bits(net.unpad(gb), g) and g.any()
    net.close()


# ---- the state of a full descriptor ------------------------------------------------------------------------------------------------------------

SECTION_NAMES = ("params", "velocity", "adam_m", "adam_v", "ema", "accum")


def _sections(net):
    """{section: its logical vector} of a snapshot of everything the net has, and the descriptor"""
    snap = net.snapshot()
    d, body = snap.desc, snap.body_bytes()
    net.synchronize()
    return {s: d.section(body, s).copy() for s in SECTION_NAMES if int(d.section_off[SECTION_NAMES.index(s)]) >= 0}, d


def _equal_per_tensor(sa, sb, tag):
    assert sorted(sa) == sorted(sb) == sorted(SECTION_NAMES), (tag, sorted(sa), sorted(sb))
    for s in SECTION_NAMES:
        for li, (ws, bs) in enumerate(tensor_slices(P32[0], P32[1])):
            assert same_bits(sa[s][ws], sb[s][ws]) and same_bits(sa[s][bs], sb[s][bs]), (tag, s, li)


def test_save_and_load_all_six_sections_and_continue_bit_for_bit(tmp_path):
    """Nesterov momentum (one step: the velocity), then Adam (its two moments), the average and accumulation by 2 with ONE micro-step
    pending: six sections over 32 jobs through k_state_pack and k_state_unpack"""
    from mercer_research_amd.convnet import ConvNet
    a, = twins(P32, "fp32", 1, sgd=NESTEROV)
    bs = batches(a, P32, 6)
    step(a, *bs[0], LR)
    a.set_adam((0.9, 0.99), 1e-4, 0.01, True)
    a.set_ema(0.9)
    a.set_accumulate(2)
    for x, y in bs[1:4]:
        step(a, x, y, 1e-2)
    assert a.get_accumulate() == (2, 1) and a.get_adam_state()[2] == 1
    path = tmp_path / "deep.state"
    a.save(path, extra=b"loop state")
    b, extra = ConvNet.load(path, P32[2])
    assert extra == b"loop state" and b.layers == [tuple(l) for l in P32[1]] and len(b.layers) == 32
    sa, da = _sections(a)
    sb, db = _sections(b)
    assert da.sections == db.sections == 63 and da.n_layers == db.n_layers == 32
    _equal_per_tensor(sa, sb, "after load")
    for li, (ws, bs_) in enumerate(tensor_slices(P32[0], P32[1])):          # no section of no layer is empty: a lost job would show
        for s in SECTION_NAMES:
            assert sa[s][ws].any(), (s, li)
    assert same_bits(stats(a), stats(b)) and b.get_accumulate() == (2, 1) and b.get_adam_state()[2] == 1
    for x, y in bs[4:]:
        step(a, x, y, 1e-2)
        step(b, x, y, 1e-2)
    sa2, sb2 = _sections(a)[0], _sections(b)[0]
    _equal_per_tensor(sa2, sb2, "two steps later")
    assert not same_bits(sa2["params"], sa["params"]) and same_bits(stats(a), stats(b)) and a.get_accumulate() == b.get_accumulate() == (2, 1)
    _close(a, b)


# ---- exact nets: P17 (one prep launch, 32 jobs) and P18 (a copy in front of every bf16 launch) ------------------------------------------------

@pytest.mark.parametrize("precision", ["fp32", "bf16"])
@pytest.mark.parametrize("name", sorted(EXACT_NETS))
def test_exact_nets_against_the_oracle(name, precision):
    """Logits bit for bit, gradients per tensor at tests/_exact_nets.py's tolerance; a second gradients call and a replayed train_step give
    the first one's bits -- P18 in bf16 makes every launch's operand copy again on every call, into one scratch that capture must see at
    its final size."""
    import torch
    spec = EXACT_NETS[name]
    in_shape, layers, B = spec
    x, y, _, _, flat = exact_case(name)
    loss_ref, logits_ref, grad_ref = exact_reference(name, precision)
    want = logits_ref.astype(np.float32)
    net = make_net(spec, precision)
    text = net.plan_of_this_net(B)
    assert ("k_prep_all_bf16" in text) == (precision == "bf16" and name == "P17") and ("k_prep_weights_bf16" in text) == (precision == "bf16" and name == "P18"), text
    net.set_params(flat)
    xd, yd = dev(net, x.copy()), dev(net, y.copy())          # (the shared case is read-only)
    g, loss, z = grads(net, xd, yd, B)
    with torch.cuda.stream(net.stream):
        ze = net.forward(xd)
    net.synchronize()
    assert same_bits(z, want) and same_bits(ze.cpu().numpy(), want), (np.abs(z - want).max(), np.abs(ze.cpu().numpy() - want).max())
    rtol = MODES[precision][1]
    assert abs(loss - loss_ref) <= rtol * max(1.0, loss_ref), (loss, loss_ref)
    close_per_tensor(g, grad_ref, in_shape, layers, rtol)
    g2, loss2, z2 = grads(net, xd, yd, B)
    assert same_bits(g2, g) and loss2 == loss and same_bits(z2, z)
    after = []
    for _ in range(3):                                    # (the first is eager, the others replay its graph)
        net.set_params(flat)
        step(net, xd, yd, EXACT_LR)
        after.append(net.get_params())
    assert same_bits(after[0], after[1]) and same_bits(after[0], after[2]) and net.graphs_instantiated() >= 1
    close_per_tensor(after[0], flat.astype(np.float64) - EXACT_LR * grad_ref, in_shape, layers, rtol)
    net.close()


def test_p18_bf16_twins_stay_bit_identical_with_overlap_on_one():
    a, b = twins(P18, "bf16", 2, sgd=(0.9, 0.0, False))
    b.set_overlap(1)
    for x, y in batches(a, P18, 3):
        step(a, x, y, LR)
        step(b, x, y, LR)
    assert _same(_state(a), _state(b)) and a.get_velocity().any() and np.isfinite(a.get_params()).all()
    _close(a, b)


# ---- bf16 on the batch-normalised deep nets: device against device -----------------------------------------------------------------------------

@pytest.mark.parametrize("name", ["P32", "RES20"])
def test_bf16_twins_agree_replay_equals_eager_and_all_is_finite(name):
    spec = DEEP_NETS[name]
    a, b = twins(spec, "bf16", 2, sgd=(0.9, 0.0, False))
    assert "k_prep_all_bf16" in a.plan_of_this_net(spec[2])
    bs = batches(a, spec, 3)
    ga, la, za = grads(a, *bs[0], spec[2])
    gb, lb, zb = grads(b, *bs[0], spec[2])
    assert same_bits(ga, gb) and la == lb and same_bits(za, zb) and np.isfinite(ga).all() and np.isfinite(za).all() and np.isfinite(la)
    for ws, _ in tensor_slices(spec[0], spec[1]):
        assert ga[ws].any()
    p0, s0 = a.get_params(), stats(a)
    eager = None
    for k in range(2):                                    # the same step twice from the same state: eager, then the replayed graph
        a.set_params(p0)
        a.set_bn_stats(s0)
        a.reset_velocity()
        step(a, *bs[0], LR)
        if k == 0:
            eager = _state(a)
    assert _same(_state(a), eager) and a.graphs_instantiated() >= 1
    b.set_bn_stats(s0)
    step(b, *bs[0], LR)
    assert _same(_state(a), _state(b))
    for x, y in bs[1:]:
        step(a, x, y, LR)
        step(b, x, y, LR)
    assert _same(_state(a), _state(b)) and all(np.isfinite(v).all() for v in _state(a)) and a.get_velocity().any()
    _close(a, b)


# ---- the 33rd layer with parameters ------------------------------------------------------------------------------------------------------------

def test_create_refuses_what_the_plan_refuses():
    """describe_layers is one function: rcn_hipx_create returns the plan's status and message, before anything is enqueued"""
    from mercer_research_amd import convnet
    in_shape, layers, B = P33
    with pytest.raises(convnet.ConvNetError) as plan_err:
        convnet.plan(in_shape, layers, B)
    with pytest.raises(convnet.ConvNetError) as create_err:
        convnet.ConvNet(in_shape, layers, B)
    assert str(plan_err.value) == "rcn_hipx_plan: -3: " + str(create_err.value).split("rcn_hipx_create: -3: ", 1)[1]
    assert "33 layers with parameters" in str(create_err.value) and "at most 32" in str(create_err.value)
