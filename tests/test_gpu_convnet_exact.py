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
Tolerances are the project's (tests/test_gpu_convnet_forms.py): 2e-4 in fp32, 5e-3 with bf16 operands or storage."""
import numpy as np
import pytest
from _convnet_util import FUSED_HEAD, PLAIN_HEAD, POOL_PAIRS, close_per_tensor, dev, make_net, same_bits, zeros
from _exact_nets import EVAL_ROWS, eval_set, exact_case, gpu_cases, reference
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
