"""GPU tests of the layer kernels' forms that no small net selects by default (cases: tests/_forms_cases.py; tests/test_convnet_forms_plan.py
proves on the CPU that each case reaches the forms it names):
  A  the looping kernels (launch_resident: k_conv3x3_halo_f32, k_conv1_fwd_f32, k_conv3x3_halo_bf16p, k_conv3x3_halo_bf16_1cb) on grids of
     1, 2, 3, 5 and 7 workgroups ("halo_f32_slots"), so that every workgroup takes several items: the mixed-radix advance() with its
     carries, the barrier that guards LDS reuse between items, the prefetch of the next item's halo, the 1cb kernel's reload of weights
     and bias registers.  An item's arithmetic does not depend on which workgroup runs it: bit for bit the one-item-per-workgroup run,
     which is held by the oracle.
  B  more than one pixel block per chunk of the LDS-tiled weight gradients (the block loop with the next block's loads in flight).  The
     order of the sums changes with the chunk size: against the oracle, and a second evaluation bit-identical.
  C  forms only an option selects, each against the oracle in its mode; where the option changes the schedule alone, bit for bit too.
Tolerances are the project's: fp32 vs f64 2e-4 of scale + 1e-6 (4e-4 after a second step; tests/test_gpu_convnet.py); bf16 operands vs the
oracle with the same operand rounding 5e-3 (2e-2 after two steps); bf16 storage vs the oracle with the storage rounding mirrored 5e-3
(2e-2 after two steps; tests/test_gpu_convnet_bf16_stored.py).  In every mode the gradient and the parameters after one step are held tensor by
tensor, each layer's weights and each layer's biases at their own scale (close_per_tensor).  A parameter vector after ONE step is held
at the gradient's tolerance: it is the parameters (exact) minus LR times a gradient within that tolerance; so is that step's displacement
(check_oracle)."""
import functools
from types import SimpleNamespace

import numpy as np
import pytest
from _convnet_util import make_net, oracle_params, same_bits
from _forms_cases import LOOPS, OPTIONS, SLOTS, WGRADS, names
from _oracle_steps import KEYS, LR, MODES, check_oracle, run

from oracle import convnet_oracle as co

pytestmark = pytest.mark.gpu


@functools.lru_cache(maxsize=None)
def reference(spec, precision):
    """Parameters, one batch and the oracle's logits, loss, gradient and two SGD steps in `precision`'s mode, computed once per (net,
    mode) and shared by the cases on it; the arrays are read-only."""
    in_shape, layers, B = spec
    kw = MODES[precision][0]
    rng = np.random.default_rng(B + in_shape[0])
    _, _, flat, w32, b32 = oracle_params(rng, in_shape, layers)
    x = rng.standard_normal((B,) + in_shape).astype(np.float32)
    y = rng.integers(0, layers[-1][1], B).astype(np.int32)
    x64 = x.astype(np.float64)
    loss, logits, gws, gbs = co.loss_and_grads(x64, y, w32, b32, layers, **kw)
    w1, b1, _ = co.sgd_step(x64, y, w32, b32, layers, LR, **kw)
    w2, b2, loss1 = co.sgd_step(x64, y, w1, b1, layers, LR, **kw)
    ref = SimpleNamespace(flat=flat.astype(np.float32), x=x, y=y, logits=logits, loss=loss, grad=co.flatten(gws, gbs), params1=co.flatten(w1, b1),
                          params2=co.flatten(w2, b2), loss1=loss1, spec=spec)
    for a in vars(ref).values():
        if isinstance(a, np.ndarray):
            a.setflags(write=False)
    return ref


def setup(case):
    """the case's net with its options set (its plan names the promised forms), its reference, its batch on the device"""
    ref = reference(case.spec, case.precision)
    net = make_net(case.spec, precision=None, tiling=case.tiling)
    for name, value in case.options.items():
        net.set_option(name, value)
    net.set_precision(case.precision)
    L = net.plan_of_this_net(case.spec[2]).splitlines()
    for text in case.lines:
        assert any(names(l, text) for l in L), (text, L)
    xd, yd = net.to_device(ref.x.copy()), net.to_device(ref.y.copy())      # (the reference's arrays are read-only)
    net.synchronize()
    return net, ref, xd, yd


def assert_same_bits(tag, got, want):
    for k in KEYS:
        assert same_bits(got[k], want[k]), (tag, k, float(np.abs(got[k].astype(np.float64) - want[k]).max()), int((got[k] != want[k]).sum()))


@pytest.mark.parametrize("case", LOOPS, ids=[c.id for c in LOOPS])
def test_looping_changes_nothing_but_the_schedule(case):
    net, ref, xd, yd = setup(case)
    net.set_option("halo_f32_slots", 0)               # the grid is the items: far fewer than the chip's slots
    base = run(net, ref, xd, yd)
    check_oracle(base, ref, case.precision)
    plan = net.plan_of_this_net(case.spec[2])
    for s in SLOTS:
        net.set_option("halo_f32_slots", s)
        assert net.plan_of_this_net(case.spec[2]) == plan
        assert_same_bits(f"{s} workgroups", run(net, ref, xd, yd), base)
    net.close()


@pytest.mark.parametrize("case", WGRADS, ids=[c.id for c in WGRADS])
def test_weight_gradient_chunks_of_several_pixel_blocks_match_oracle(case):
    """the oracle on every case (on the first layer's too: its net costs the oracle well under a second)"""
    import torch
    net, ref, xd, yd = setup(case)
    out = run(net, ref, xd, yd)
    check_oracle(out, ref, case.precision)
    net.set_params(ref.flat)
    with torch.cuda.stream(net.stream):
        again = net.gradients(xd, yd)
    net.synchronize()
    assert same_bits(again.cpu().numpy(), out["grad"])    # fixed summation orders
    net.close()


@pytest.mark.parametrize("case", OPTIONS, ids=[c.id for c in OPTIONS])
def test_option_selected_forms_match_oracle(case):
    net, ref, xd, yd = setup(case)
    out = run(net, ref, xd, yd)
    check_oracle(out, ref, case.precision)
    if case.twin:
        # the same arithmetic in another schedule (xcd_remap: another block order) or another kernel of the same LDS images, rounding and
        # MFMA order (bf16_pipe: select_conv's claim)
        for name, value in case.twin.items():
            net.set_option(name, value)
        assert_same_bits(f"twin {case.twin}", run(net, ref, xd, yd), out)
    net.close()
