"""GPU tests of Track X's global average pooling (include/rcn_hipx.h: RCN_HIPX_GLOBAL_AVGPOOL; csrc/convnet_gap.hpp: k_gap_fwd,
k_gap_bwd<GATE>) on the nets of tests/test_convnet_gap_plan.py: against PyTorch on the CPU in float64 (tests/_torch_ref.py) -- the logits of
a training forward, the loss, the gradients per tensor, parameters and running statistics after plain SGD steps, the forward and the
evaluation; bit for bit on integer nets whose sums and quotients are exact; the gate for the ReLU below the pool; and the layer inside the
recipe (twins, overlap, buckets, the epoch's one graph, metrics, save / load, dropout).

Tolerances are those of tests/test_gpu_convnet_res.py: fp32 against f64 2e-4 of a tensor's scale + 1e-6, 4e-4 after a second step; bf16
operands 5e-3 / 2e-2 against the twin with the SAME operand rounding, the training logits also 3e-2 against the unrounded twin."""
import numpy as np
import pytest
from _convnet_util import LR, batches, close, dev, epoch, make_net, same_bits, step, twins
from _gap_cases import exact_forward, exact_gate_case, exact_logit_case, rows_seen
from _torch_ref import TorchNet, close_per_tensor, tensor_slices
from _twin_checks import compare, device_run, grads as _grads, stats as _stats
from test_convnet_gap_plan import (EXACT_SHAPES, GAP_A, GAP_B, GAP_C, GAP_LOOP, GAP_NETS, GATE_PIXELS, RTOL, RTOL_2, SEEDS, STEPS, data, gate_case,
                                   twin_run)

pytestmark = pytest.mark.gpu

CASES = [(n, p) for n in sorted(GAP_NETS) for p in ("fp32", "bf16")]
LAYERS = (("conv", 32), ("global_avgpool",), ("dense", 10))         # of the exact nets


def _run(name, precision, tiling=None, options=()):
    """What the device makes of twin_run's schedule: one gradients call, STEPS plain SGD steps, a forward and an evaluation"""
    spec = GAP_NETS[name]
    return device_run(spec, precision, *data(spec, SEEDS[name]), STEPS, tiling=tiling, options=options)


def _compare(name, precision, r, tag=""):
    """every comparison of tests/_twin_checks.py: compare; returns the worst share of an allowance"""
    spec = GAP_NETS[name]
    unrounded = None
    if precision == "bf16":
        flat, x, y = data(spec, SEEDS[name])
        unrounded = (TorchNet(spec[0], spec[1], flat).logits(x, train=True), 3e-2)
    return compare(spec, r, twin_run(name, precision), RTOL[precision], RTOL_2[precision], STEPS, f"{name} {precision}{tag}", unrounded)


@pytest.mark.parametrize("name,precision", CASES, ids=[f"{n}-{p}" for n, p in CASES])
def test_against_the_twin(name, precision):
    _compare(name, precision, _run(name, precision))


@pytest.mark.parametrize("fuse", [0, 1])
def test_net_c_with_the_pool_backward_fused_and_not(fuse):
    """net c on the LDS-tiled kernels: the max-pool below the global average pool hands its gradient to k_pool_bwd (0) or to the
    convolution's gradient kernels, which unpool while staging (1) -- the pool's dout, written ungated by k_gap_bwd, is complete either way"""
    from mercer_research_amd import convnet
    net = make_net(GAP_C, "fp32", tiling="lds")
    net.set_option("fuse_pool_bwd", fuse)
    text = net.plan_of_this_net(GAP_C[2])
    net.close()
    assert ("k_pool_bwd" in text) == (fuse == 0) and "ungated: layer 1 is a pool" in text, text
    _compare("c", "fp32", _run("c", "fp32", tiling="lds", options=(("fuse_pool_bwd", fuse),)), tag=f" lds fuse_pool_bwd={fuse}")
    assert convnet.KIND["global_avgpool"] == 7


def test_loop_case_against_the_twin():
    """B = 8200: k_gap_bwd's capped grid takes a second grid-stride trip (tests/test_convnet_gap_plan.py proves it from the plan)"""
    in_shape, layers, B = GAP_LOOP
    flat, x, y = data(GAP_LOOP, 5)
    net = make_net(GAP_LOOP, "fp32")
    net.set_params(flat)
    g, loss, z = _grads(net, dev(net, x), dev(net, y), B)
    net.close()
    rloss, rz, rg = TorchNet(in_shape, layers, flat).loss_and_grads(x, y)
    close(z, rz, RTOL["fp32"], "loop training logits")
    close([loss], [rloss], RTOL["fp32"], "loop loss")
    close_per_tensor(g, rg, in_shape, layers, RTOL["fp32"], "loop gradient")


# ---- exact ----------------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", sorted(EXACT_SHAPES))
def test_exact_logits_bit_for_bit(name):
    """positive integer maps, HW a power of two: every sum and the division are exact (tests/test_convnet_gap_plan.py), so the training
    logits and the forward logits ARE the NumPy result"""
    import torch
    in_shape, C, classes, B = EXACT_SHAPES[name]
    x, y, w0, b0, w1, b1, flat = exact_logit_case(in_shape, C, classes, B)
    want = exact_forward(x, w0, b0, w1, b1)[2].astype(np.float32)
    net = make_net((in_shape, LAYERS, B), "fp32")
    net.set_params(flat)
    xd, yd = dev(net, x), dev(net, y)
    _, _, z = _grads(net, xd, yd, B)
    with torch.cuda.stream(net.stream):
        ze = net.forward(xd)
    net.synchronize()
    net.close()
    assert same_bits(z, want) and same_bits(ze.cpu().numpy(), want), np.abs(z - want).max()


@pytest.mark.parametrize("name", sorted(EXACT_SHAPES))
def test_exact_input_gradient_is_g_over_hw_or_zero(name):
    """One sample with one non-zero input value (tests/_gap_cases.py: exact_gate_case): the dense layer's bias gradient IS d logits, the pool's
    gradient is g[c] = +-1/2 of ONE d logit, and the first convolution's weight gradient at (tap, channel 0) has ONE non-zero term -- the
    pool's input gradient at the row that tap reaches from the pixel: fl(g[c] / HW) where the map is positive there, 0 where the ReLU is shut."""
    in_shape, C, classes, _ = EXACT_SHAPES[name]
    HW = in_shape[0] * in_shape[1]
    spec = (in_shape, LAYERS, 1)
    (ws0, _), (_, bs1) = tensor_slices(in_shape, LAYERS)
    net = make_net(spec, "fp32")
    checked = 0
    for k, pixel in enumerate(GATE_PIXELS[name]):
        x, y, w0, b0, w1, b1, flat = exact_gate_case(in_shape, C, classes, pixel, seed=k)
        a = exact_forward(x, w0, b0, w1, b1)[0]
        net.set_params(flat)
        g, _, _ = _grads(net, dev(net, x), dev(net, y), 1)
        dlog = g[bs1].astype(np.float32)
        assert dlog.any()
        gpool = (w1.astype(np.float32) * dlog[None, :]).sum(1, dtype=np.float32)           # one non-zero term per row: exact
        share = gpool / np.float32(HW)                                                    # a power of two: exact
        dw = g[ws0].reshape(9, in_shape[2], C)
        rows = rows_seen(in_shape, pixel)
        for tap in range(9):
            want = np.where(a[0, rows[tap]] > 0, share, np.float32(0)) if tap in rows else np.zeros(C, dtype=np.float32)
            assert np.array_equal(dw[tap, 0], want), (pixel, tap, dw[tap, 0], want)
            checked += int(tap in rows)
        assert not dw[:, 1:].any()                                                        # the other input channels are zero
    net.close()
    assert checked == sum(len(rows_seen(in_shape, p)) for p in GATE_PIXELS[name])


# ---- the gate -------------------------------------------------------------------------------------------------------------------------------

def test_the_gate_is_seen():
    """net a: the device's gradient agrees with the honest twin within the bounds and is many allowances away from the twin that drops the
    ReLU below the pool on the gradient path (tests/test_convnet_gap_plan.py shows the two twins apart and the share of closed gates)"""
    in_shape, layers, B = GAP_A
    flat, x, y = gate_case()
    net = make_net(GAP_A, "fp32")
    net.set_params(flat)
    g, _, _ = _grads(net, dev(net, x), dev(net, y), B)
    net.close()
    _, _, g_true = TorchNet(in_shape, layers, flat).loss_and_grads(x, y)
    _, _, g_loose = TorchNet(in_shape, layers, flat, gate_below=False).loss_and_grads(x, y)
    close_per_tensor(g, g_true, in_shape, layers, RTOL["fp32"], "net a, gated below the pool: gradient")
    ws, bs = tensor_slices(in_shape, layers)[0]
    factor = max(float(np.abs(g[t] - g_loose[t]).max()) / (2e-4 * max(1e-3, float(np.abs(g_loose[t]).max())) + 1e-6) for t in (ws, bs))
    print(f"against the twin without the gate: worst |d| / allowance = {factor:.1f}")
    assert factor > 100.0, factor


# ---- bits -----------------------------------------------------------------------------------------------------------------------------------

def _state(net):
    return net.get_params(), _stats(net), net.get_velocity()


def _same(a, b):
    return all(same_bits(u, v) for u, v in zip(a, b))


def _close(*nets):
    for n in nets:
        n.close()


@pytest.mark.parametrize("name", ["b", "c"])
@pytest.mark.parametrize("overlap", [0, 1])
def test_twins_are_bit_identical(name, overlap):
    """two contexts of one net hold the same bits; with overlap the second context runs its weight gradients on the side stream"""
    spec = GAP_NETS[name]
    a, b = twins(spec, "fp32", 2, sgd=(0.9, 0.0, False))
    b.set_overlap(overlap)
    bs = batches(a, spec, 3)
    ga, la, za = _grads(a, *bs[0], spec[2])
    gb, lb, zb = _grads(b, *bs[0], spec[2])
    assert same_bits(ga, gb) and la == lb and same_bits(za, zb)
    for x, y in bs:
        step(a, x, y, LR)
        step(b, x, y, LR)
    assert _same(_state(a), _state(b)) and a.get_velocity().any()
    _close(a, b)


@pytest.mark.parametrize("name", ["b", "c"])
def test_buckets_around_the_pool_change_no_bit(name):
    """at 0 bytes every layer with parameters is a bucket: one boundary lies directly above the pool (the dense layer wrote its dout in
    the bucket before), and the pool opens the bucket of the layer below it -- a bucket cannot END with the pool, which has no parameters"""
    import torch
    spec = GAP_NETS[name]
    net, = twins(spec, "fp32", 1)
    x, y = batches(net, spec, 1)[0]
    g, _, _ = _grads(net, x, y, spec[2])
    gb = torch.zeros(net.n_padded, dtype=torch.float32, device=net.device)
    seen = []
    with torch.cuda.stream(net.stream):
        net.gradients_bucketed(x, y, gb, min_bucket_bytes=0, on_bucket=lambda *a: seen.append(a))
    net.synchronize()
    assert len(seen) >= 2 and same_bits(net.unpad(gb), g)
    net.close()


def test_epoch_equals_steps_on_one_graph():
    in_shape, layers, B = GAP_A
    a, b = twins(GAP_A, "fp32", 2)
    rng = np.random.default_rng(2)
    n = 3 * B
    X, y = rng.standard_normal((n,) + in_shape).astype(np.float32), rng.integers(0, 10, n).astype(np.int32)
    perm = rng.permutation(n).astype(np.int32)
    epoch(a, dev(a, X), dev(a, y), dev(a, perm), B, LR)
    for s in range(3):
        rows = perm[s * B:(s + 1) * B]
        step(b, dev(b, X[rows]), dev(b, y[rows]), LR)
    assert _same(_state(a), _state(b))
    assert a.graphs_instantiated() == 1
    _close(a, b)


def test_metrics_agree_with_evaluate_and_forward():
    import torch
    in_shape, layers, B = GAP_B
    net, = twins(GAP_B, "fp32", 1)
    x, y = batches(net, GAP_B, 1)[0]
    step(net, x, y, LR)                                    # (running statistics that are not their defaults)
    loss, correct = net.evaluate(x, y, x_scale=1.0, x_shift=0.0)
    rep = net.evaluate_metrics(x, y, topk=(1, 5), logits=True, x_scale=1.0, x_shift=0.0)
    with torch.cuda.stream(net.stream):
        z = net.forward(x)
    net.synchronize()
    assert rep.loss == loss and rep.correct == correct and rep.topk[1] == correct
    assert same_bits(rep.logits, z.cpu().numpy())
    net.close()


def test_save_and_load_rebuild_the_description_and_continue_bit_for_bit(tmp_path):
    from mercer_research_amd.convnet import ConvNet
    a, = twins(GAP_B, "fp32", 1, sgd=(0.9, 5e-4, True))
    bs = batches(a, GAP_B, 3)
    for x, y in bs[:2]:
        step(a, x, y, LR)
    path = tmp_path / "gap.state"
    a.save(path, extra=b"loop state")
    b, extra = ConvNet.load(path, GAP_B[2])
    assert extra == b"loop state" and b.layers == [tuple(l) for l in GAP_B[1]] and b.layers[6] == ("global_avgpool",)
    assert _same(_state(a), _state(b))
    step(a, *bs[2], LR)
    step(b, *bs[2], LR)
    assert _same(_state(a), _state(b))
    _close(a, b)


def test_dropout_has_one_site_behind_the_pool_and_twins_stay_equal():
    a, b = twins(GAP_B, "fp32", 2)
    for n in (a, b):
        n.set_dropout(0.5, 7)
    assert a.get_dropout()[2] == 1
    plain, = twins(GAP_B, "fp32", 1)
    for x, y in batches(a, GAP_B, 3):
        step(a, x, y, LR)
        step(b, x, y, LR)
        step(plain, x, y, LR)
    assert _same(_state(a), _state(b)) and a.dropout_state() == 3
    assert not same_bits(a.get_params(), plain.get_params())          # the masks did something
    _close(a, b, plain)


def test_bf16_stored_is_refused_and_changes_nothing():
    from mercer_research_amd import convnet
    a, b = twins(GAP_A, "bf16", 2)
    with pytest.raises(convnet.ConvNetError, match=r"status -3.*RCN_HIPX_BF16_STORED.* does not cover global average pooling"):
        a.set_precision("bf16_stored")
    assert "bf16 operand copies" in a.plan_of_this_net(GAP_A[2]) and "stored as bf16" not in a.plan_of_this_net(GAP_A[2])
    for x, y in batches(a, GAP_A, 2):
        step(a, x, y, LR)
        step(b, x, y, LR)
    assert _same(_state(a), _state(b))
    _close(a, b)


def test_create_refuses_what_the_plan_refuses():
    """describe_layers is one function: rcn_hipx_create returns the plan's status and message"""
    from mercer_research_amd import convnet
    from test_convnet_gap_plan import REFUSALS
    for layers, status, _ in REFUSALS:
        with pytest.raises(convnet.ConvNetError) as plan_err:
            convnet.plan((4, 4, 32), layers, 2)
        with pytest.raises(convnet.ConvNetError) as create_err:
            convnet.ConvNet((4, 4, 32), layers, 2)
        assert str(plan_err.value) == f"rcn_hipx_plan: {status}: " + str(create_err.value).split(f"rcn_hipx_create: {status}: ", 1)[1]
