"""GPU tests of Track X on nets whose arithmetic is exact (tests/_exact_nets.py; tests/test_convnet_exact_nets.py proves on the CPU, from
the oracle alone, everything these tests assume about their data).  Integer inputs, weights in {-1, 0, 1}, integer biases: every forward
sum is exact in fp32 in any order and survives bf16 rounding, so the device's logits must equal the oracle's BIT FOR BIT, in every
precision mode and on every kernel form -- a dropped, duplicated or mis-indexed term shows, however small.  And such data does what
Gaussian data never does: pooling windows tie at a positive maximum, pre-activations are exactly 0, the softmax saturates.
  A  forward, bit for bit: the nets of tests/test_gpu_convnet.py (auto tiling: implicit GEMM, split-K, k_pool_fwd) in fp32 and in bf16,
     the nets of tests/test_gpu_convnet_halo.py with tiling "lds", POOL_PAIRS in fp32 and bf16 storage, every case of tests/_forms_cases.py
     with its own options (the looping ones also on a grid of 2 workgroups), one net with max_batch above the batch.  Then, forward
     only, every one of these nets (the forms nets without options) in bf16 and, where the library accepts the net, under bf16 storage
     (_exact_nets.STORED_TILING; the others are refused: not every convolution of theirs runs LDS-tiled with its pool fused).  Every
     net is certified in every mode: the 8-conv net is thinned (fewer non-zeros per column in its deeper layers) for that.  The plain
     cases' plans are held to the families they are here for (_exact_nets.PLAIN_LINES), as the forms cases' are.
     Per precision, the forward families of select_conv: k_conv1_fwd_f32 halo-*, convnet-bf16-0,
     forms-stored-*; k_conv3x3_halo_f32 halo-*, forms-fp32-*; k_conv_fwd convnet-*-fp32, forms-xcd-remap-fp32-*; k_conv3x3_halo_bf16p
     convnet-bf16-0, forms-stored-pipelined; k_conv3x3_halo_bf16_1cb forms-bf16-1cb-reload, forms-stored-1cb; k_conv3x3_halo_bf16
     forms-bf16-not-pipelined(-plain); k_conv_fwd_bf16 forms-bf16-no-lds-tiling and every bf16 dense layer; its bf16-map form
     forms-stored-*, pool-pairs-stored.  The 16-row form of k_conv3x3_halo_bf16p needs 512 work items of 16 x 16 pixels: no small net
     reaches it, and it stays with the workload-size tests.
  B  evaluate / predict over an exact uint8 set: the arg-max (first maximum) and the correct count exactly.
  C  backward with ties and zeros, same cases (the forms cases thinned to _exact_nets.FORMS_BACKWARD): gradients tensor by tensor
     against the oracle in the case's mode, one eager and one replayed step, a second evaluation bit-identical.
  D  a saturated softmax (logit gaps of 160 to 176, where expf underflows to 0): k_head_f32, k_softmax_ce and the 40-class lane loop,
     plain and smoothed, and a pair step.
  E  the backward pass BIT FOR BIT (_exact_nets.BACKWARD_CASES): nets whose softmax is exact too -- t classes tied at the maximum, the
     others 120 or more below, a power-of-two batch -- so that d logits, every dZ, every weight and bias gradient and the parameters
     after a step at a power-of-two rate are small multiples of powers of two.  The device's gradient must EQUAL the f64 reference's in
     every element, in fp32, bf16 and bf16 storage alike; so must the parameters after one eager and one replayed step, after a step
     with momentum, weight decay and Nesterov (with the velocity), the average under set_ema, the accumulator and the parameters under
     set_accumulate(2), and the soft targets of set_loss(0.125) and a pair step at weight 0.25.  No tolerance but the loss's (logf).
Tolerances are the project's (tests/test_gpu_convnet_forms.py): 2e-4 in fp32, 5e-3 with bf16 operands or storage."""
import numpy as np
import pytest
from _convnet_util import FUSED_HEAD, PLAIN_HEAD, POOL_PAIRS, close_per_tensor, dev, make_net, same_bits, tensor_slices, zeros
from _exact_nets import (ACCUM, BACKWARD_CASES, EMA, EVAL_ROWS, PAIR_W, SGD, SMOOTH, STEP_LR, backward_case, eval_set, exact_case, gpu_cases, reference)
from _forms_cases import DENSE_NK, names
from _mix_ref import soft_loss_and_grads, soft_loss_f64, soft_targets
from _oracle_steps import LR, check_oracle, close_loss, run

from oracle import convnet_oracle as co

pytestmark = pytest.mark.gpu

CASES = gpu_cases()


def first_argmax(logits):
    return np.argmax(logits, axis=1).astype(np.int32)               # (np.argmax: the first maximum)


def assert_logits_bit_for_bit(got, want64):
    want = want64.astype(np.float32)
    if not same_bits(got, want):
        bad = np.argwhere(got.view(np.uint32) != want.view(np.uint32))
        raise AssertionError(f"{len(bad)} of {want.size} logits differ; the first at {tuple(bad[0])}: device {got[tuple(bad[0])]!r}, oracle {want[tuple(bad[0])]!r}")


# ---- A and C ---------------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("case", CASES, ids=[c.id for c in CASES])
def test_exact_net_logits_bit_for_bit_and_gradients_with_ties_and_zeros(case):
    import torch
    in_shape, layers, B = case.spec
    ref = reference(case.spec, case.precision, LR, case.backward)
    net = make_net(case.spec, precision=None, tiling=case.tiling, max_batch=case.max_batch)
    for name, value in case.options.items():
        net.set_option(name, value)
    if case.slots is not None:
        net.set_option("halo_f32_slots", case.slots)
    net.set_precision(case.precision)
    L = net.plan_of_this_net(B).splitlines()
    for text in case.lines:
        assert any(names(l, text) for l in L), (text, L)
    net.set_params(ref.flat)
    assert same_bits(net.get_params(), ref.flat)
    xd, yd = dev(net, ref.x.copy()), dev(net, ref.y.copy())         # (the reference's arrays are read-only)
    with torch.cuda.stream(net.stream):
        logits = net.forward(xd)
    net.synchronize()
    assert_logits_bit_for_bit(logits.cpu().numpy(), ref.logits)
    if case.backward:
        out = run(net, ref, xd, yd)                                  # logits, loss, gradient; one eager and one replayed step
        assert_logits_bit_for_bit(out["logits"], ref.logits)
        assert np.isfinite(out["grad"]).all()
        check_oracle(out, ref, case.precision)
        net.set_params(ref.flat)
        with torch.cuda.stream(net.stream):
            again = net.gradients(xd, yd)
        net.synchronize()
        assert same_bits(again.cpu().numpy(), out["grad"])
    net.close()


# ---- B ---------------------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("spec", [FUSED_HEAD, PLAIN_HEAD, POOL_PAIRS], ids=["fused_head", "plain_head", "pool_pairs"])
def test_evaluation_over_an_exact_uint8_set(spec):
    _, layers, B = spec
    case = exact_case(spec)
    Xh, yh = eval_set(spec)
    assert EVAL_ROWS[spec] % B
    logits = co.forward(Xh.astype(np.float64) - 2.0, list(case.ws), list(case.bs), layers)
    net = make_net(spec, "fp32")
    net.set_params(case.flat)
    X, y = dev(net, Xh), dev(net, yh)
    kw = dict(x_scale=1.0, x_shift=-2.0)
    pred = net.predict(X, **kw)
    net.synchronize()
    want = first_argmax(logits)
    assert np.array_equal(pred.cpu().numpy(), want)
    loss, correct = net.evaluate(X, y, **kw)
    assert correct == int((want == yh).sum())
    close_loss("evaluate", loss, soft_loss_f64(logits, yh, yh, 1.0, 0.0), 2e-4)
    net.close()


# ---- D ---------------------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("spec,options", [(FUSED_HEAD, {}), (PLAIN_HEAD, {}), (DENSE_NK, {"head": 0})], ids=["fused_head", "plain_head", "dense_nk-40-classes"])
def test_saturated_softmax_keeps_loss_and_gradients(spec, options):
    import torch
    in_shape, layers, B = spec
    classes = layers[-1][1]
    case = exact_case(spec, "saturated")
    x64, ws, bs = case.x.astype(np.float64), list(case.ws), list(case.bs)
    yb = np.random.default_rng(7).integers(0, classes, B).astype(np.int32)
    assert ((0 <= case.y) & (case.y < classes) & (0 <= yb) & (yb < classes)).all()
    net = make_net(spec, precision=None)
    for name, value in options.items():
        net.set_option(name, value)
    net.set_precision("fp32")
    net.set_params(case.flat)
    xd, yd, ybd = dev(net, case.x.copy()), dev(net, case.y.copy()), dev(net, yb)
    w = dev(net, np.array([0.25], dtype=np.float32))
    loss = zeros(net, 1)
    with torch.cuda.stream(net.stream):
        logits = net.forward(xd)
    net.synchronize()
    assert_logits_bit_for_bit(logits.cpu().numpy(), case.logits)
    for eps in (0.0, 0.1):
        e = float(np.float32(eps))
        net.set_params(case.flat)
        net.set_loss(eps)
        with torch.cuda.stream(net.stream):
            g = net.gradients(xd, yd, loss=loss)
        net.synchronize()
        got, g = float(loss.item()), net.unpad(g)
        assert np.isfinite(got) and np.isfinite(g).all(), (eps, got)
        T = soft_targets(case.y, case.y, 1.0, e, classes)
        _, _, gws, gbs = soft_loss_and_grads(x64, T, ws, bs, layers)
        close_loss(f"smoothing {eps}", got, soft_loss_f64(case.logits, case.y, case.y, 1.0, e), 2e-4)
        close_per_tensor(g, co.flatten(gws, gbs), in_shape, layers, 2e-4)
        # a pair step at weight 0.25: its loss, and the parameters after it
        lr = 2.0 ** -6
        with torch.cuda.stream(net.stream):
            net.train_step_pair(xd, yd, ybd, w, lr, loss)
        net.synchronize()
        got, after = float(loss.item()), net.get_params()
        assert np.isfinite(got) and np.isfinite(after).all(), (eps, got)
        close_loss(f"pair step, smoothing {eps}", got, soft_loss_f64(case.logits, case.y, yb, 0.25, e), 2e-4)
        _, _, gws, gbs = soft_loss_and_grads(x64, soft_targets(case.y, yb, 0.25, e, classes), ws, bs, layers)
        close_per_tensor(after, co.flatten(ws, bs) - lr * co.flatten(gws, gbs), in_shape, layers, 2e-4)
    # evaluate: the plain cross-entropy of the same logits, whatever set_loss says
    net.set_params(case.flat)
    mean_loss, correct = net.evaluate(xd, yd)
    assert np.isfinite(mean_loss)
    close_loss("evaluate", mean_loss, soft_loss_f64(case.logits, case.y, case.y, 1.0, 0.0), 2e-4)
    assert correct == int((first_argmax(case.logits) == case.y).sum())
    net.close()


# ---- E ---------------------------------------------------------------------------------------------------------------------------------------

def tensors_differ(got, want64, spec):
    """None, or the report of the first tensor of the logical layout in which `got` (float32) and `want64` differ as values (a NaN differs;
    -0 is 0): its layer and kind, how many of its entries differ and the first of them"""
    in_shape, layers, _ = spec
    got, want64 = np.asarray(got).ravel(), np.asarray(want64, dtype=np.float64).ravel()
    assert got.dtype == np.float32 and got.size == want64.size, (got.dtype, got.size, want64.size)
    for li, pair in enumerate(tensor_slices(in_shape, layers)):
        for name, sl in zip(("weights", "biases"), pair):
            g, w = got[sl].astype(np.float64), want64[sl]
            if not np.array_equal(g, w):
                bad = np.flatnonzero(~(g == w))
                return f"parameter layer {li} {name}: {len(bad)} of {w.size} entries differ; the first at {bad[0]}: device {float(g[bad[0]])!r}, reference {float(w[bad[0]])!r}"
    return None


def assert_equal_values(what, got, want64, spec):
    report = tensors_differ(got, want64, spec)
    assert report is None, f"{what}: {report}"


def configured(case):
    net = make_net(case.spec, precision=None, tiling=case.tiling)
    for name, value in case.options.items():
        net.set_option(name, value)
    if case.slots is not None:
        net.set_option("halo_f32_slots", case.slots)
    net.set_precision(case.precision)
    return net


def one_step(net, flat, train, *args):
    """`train` (train_step or train_step_pair) once from the parameters `flat`; the parameters after it"""
    import torch
    if flat is not None:
        net.set_params(flat)
    with torch.cuda.stream(net.stream):
        train(*args)
    net.synchronize()
    return net.get_params()


def exact_gradient(net, xd, yd, loss):
    import torch
    with torch.cuda.stream(net.stream):
        g = net.gradients(xd, yd, loss=loss)
    net.synchronize()
    return g.cpu().numpy(), net.unpad(g), float(loss.item())


@pytest.mark.parametrize("case", BACKWARD_CASES, ids=[c.id for c in BACKWARD_CASES])
def test_exact_net_backward_pass_equals_the_reference_in_every_element(case):
    import torch
    in_shape, layers, B = case.spec
    ref = backward_case(case.spec, case.extra)
    net = configured(case)
    L = net.plan_of_this_net(B).splitlines()
    for text in case.lines:
        assert any(names(l, text) for l in L), (text, L)
    # 1. the forward pass, bit for bit
    net.set_params(ref.flat)
    assert same_bits(net.get_params(), ref.flat)
    xd, yd = dev(net, ref.x.copy()), dev(net, ref.y.copy())
    with torch.cuda.stream(net.stream):
        logits = net.forward(xd)
    net.synchronize()
    assert_logits_bit_for_bit(logits.cpu().numpy(), ref.logits)
    # 2. the gradient, element for element
    if case.extra == "soft":
        net.set_loss(SMOOTH)
    loss = zeros(net, 1)
    padded, g, got_loss = exact_gradient(net, xd, yd, loss)
    head_bias = tensor_slices(in_shape, layers)[-1][1]
    print("logits layer's bias gradient: device", g[head_bias], "reference", ref.grad[head_bias])
    assert np.array_equal(g[head_bias].astype(np.float64), ref.grad[head_bias]), (
        "the logits layer's bias gradient, the column sums of d = (p - T) / B, is not the reference's: the softmax premises do not hold on "
        f"this device -- expf(0) == 1, expf(x) == 0 for x <= -120, 1 / {ref.t} and 1 / {B} exact.  device {g[head_bias]!r}, reference {ref.grad[head_bias]!r}")
    assert_equal_values("gradient", g, ref.grad, case.spec)
    close_loss("loss", got_loss, ref.loss, 2e-4)
    # 3. a second pass has the same bits
    again, _, _ = exact_gradient(net, xd, yd, loss)
    assert same_bits(again, padded)
    # 4. one plain step at a power-of-two rate: eager, then the same step as a replayed graph
    if case.extra == "soft":
        net.set_loss(0.0)
        ref_plain = backward_case(case.spec, None)                   # (same seed: the same net with its hard target)
        assert np.array_equal(ref_plain.flat, ref.flat)
        want1 = ref_plain.params1
    else:
        want1 = ref.params1
    graphs = net.graphs_instantiated()
    eager = one_step(net, ref.flat, net.train_step, xd, yd, STEP_LR, loss)
    assert net.graphs_instantiated() == graphs + 1                   # (the first step of a key runs eagerly and is then captured)
    assert_equal_values("parameters after one eager step", eager, want1, case.spec)
    replayed = one_step(net, ref.flat, net.train_step, xd, yd, STEP_LR, loss)
    assert net.graphs_instantiated() == graphs + 1                   # (a replay)
    assert same_bits(replayed, eager)
    # 5. momentum, weight decay and Nesterov in the update
    if case.extra == "sgd":
        net.set_sgd(*SGD)
        net.reset_velocity()
        after = one_step(net, ref.flat, net.train_step, xd, yd, STEP_LR, loss)
        assert_equal_values("parameters after one step with momentum, weight decay and Nesterov", after, ref.sgd_params, case.spec)
        assert_equal_values("velocity after that step", net.get_velocity(), ref.sgd_velocity, case.spec)
    # 6. the average, the accumulator, the soft targets
    if case.extra == "ema":
        net.set_params(ref.flat)
        net.set_ema(EMA)                                             # (the first decay > 0 starts the average as a copy of the live parameters)
        net.reset_ema()
        after = one_step(net, None, net.train_step, xd, yd, STEP_LR, loss)
        assert same_bits(after, eager)
        assert_equal_values("average after one step", net.get_ema(), ref.ema, case.spec)
    if case.extra == "accum":
        x2d, y2d = dev(net, ref.x2.copy()), dev(net, ref.y2.copy())
        net.set_params(ref.flat)
        g2 = exact_gradient(net, x2d, y2d, loss)[1]
        assert_equal_values("gradient of the second batch", g2, ref.grad2, case.spec)
        net.set_accumulate(ACCUM)
        first = one_step(net, ref.flat, net.train_step, xd, yd, STEP_LR, loss)
        assert same_bits(first, ref.flat)                            # (a first micro-step changes nothing but the accumulator)
        assert_equal_values("accumulator after the first micro-step", net.get_accumulated(), ref.acc1, case.spec)
        after = one_step(net, None, net.train_step, x2d, y2d, STEP_LR, loss)
        assert_equal_values("parameters after the second micro-step", after, ref.accum_params, case.spec)
    if case.extra == "soft":
        net.set_loss(SMOOTH)
        ybd, w = dev(net, ref.yb.copy()), dev(net, np.array([PAIR_W], dtype=np.float32))
        after = one_step(net, ref.flat, net.train_step_pair, xd, yd, ybd, w, STEP_LR, loss)
        assert_equal_values(f"parameters after a pair step at weight {PAIR_W} under smoothing {SMOOTH}", after, ref.pair_params, case.spec)
        close_loss("pair step's loss", float(loss.item()), ref.pair_loss, 2e-4)
    net.close()


def _nets_in_several_modes():
    nets = {}
    for c in BACKWARD_CASES:
        if c.extra in (None, "sgd", "ema", "accum") and c.slots is None:
            nets.setdefault(c.spec, {}).setdefault(c.precision, c)   # the first case of the net in that mode
    return [pytest.param(tuple(by_mode.values()), id="net-of-" + next(iter(by_mode.values())).id) for by_mode in nets.values() if len(by_mode) > 1]


@pytest.mark.parametrize("cases", _nets_in_several_modes())
def test_exact_gradient_is_one_array_in_every_precision_mode(cases):
    """What E's construction promises of the DEVICE, held apart from the reference: the same parameters and batch give the same gradient in
    fp32, with bf16 operands and under bf16 storage.  Where this holds and the test above fails in every mode, look at the premises (the
    softmax) or the reference; where this fails, at the kernels of the mode that stands apart."""
    grads = {}
    for case in cases:
        ref = backward_case(case.spec, None)
        net = configured(case)
        net.set_params(ref.flat)
        xd, yd = dev(net, ref.x.copy()), dev(net, ref.y.copy())
        grads[case.precision] = exact_gradient(net, xd, yd, zeros(net, 1))[1]
        net.close()
    first, *others = grads
    for mode in others:
        report = tensors_differ(grads[mode], grads[first].astype(np.float64), cases[0].spec)
        assert report is None, f"{mode} against {first}: {report}"
