"""GPU tests of the Track-X update launch as ONE kernel template (csrc/convnet_update.hpp, k_reduce_update<CLIP, SGD, EMA, DLR>): every
one of its sixteen instantiations, over the layers' slabs and over a summed buffer read as one-chunk slabs, bit for bit; and the plan text
of every configuration against what the library printed before the sixteen named kernels became one template.

The twin-net method of tests/test_gpu_convnet_clip.py.  tests/golden/update_plans.json was recorded on an MI355X with the
library of the commit BEFORE the template (`python tests/test_gpu_convnet_update_forms.py OUT.json` with that commit's package on the
path): it is the yardstick, never regenerate it from the code under test."""
import itertools
import json
import os
import sys

import numpy as np
import pytest
from _accum_ref import accumulate
from _clip_ref import apply_coef, grad_norm, plain_update
from _convnet_util import FUSED_HEAD, NESTEROV, PLAIN, PLAIN_HEAD, batch, check_norm, grad, make_net, same_bits, step, twins
from _ema_ref import ema_update
from _sgd_ref import sgd_update

pytestmark = pytest.mark.gpu

DECAY = 0.9
LRS = [0.05, 0.05, 0.02, 0.05]                          # eager, replay, a second rate, back to the first
FORMS = list(itertools.product([False, True], [False, True], [False, True], [1, 2]))      # (clip, sgd, ema, accumulate)
FORM_IDS = [("clip" if c else "noclip") + ("-sgd" if s else "-plain") + ("-ema" if e else "-noema") + f"-acc{k}" for c, s, e, k in FORMS]


def _configure(net, sgd, ema, k):
    if sgd:
        net.set_sgd(*NESTEROV)
    if ema:
        net.set_ema(DECAY)
    if k > 1:
        net.set_accumulate(k)


@pytest.mark.parametrize("clip,sgd,ema,k", FORMS, ids=FORM_IDS)
def test_train_step_is_the_host_update_bit_for_bit(clip, sgd, ema, k):
    """four updates (of k micro-batches each, every one with its own data) against the NumPy restatements: the rate from the host"""
    spec = PLAIN_HEAD
    a, b = twins(spec, "fp32")
    _configure(a, sgd, ema, k)
    opt = NESTEROV if sgd else PLAIN
    batches = [batch(a, spec, 20 + j) for j in range(k)]
    p = a.get_params()
    v, e = np.zeros(a.n_logical, dtype=np.float32), p.copy()
    max_norm = None
    if clip:
        first = [grad(b, x, y, p)[1] for x, y in batches]
        max_norm = float(grad_norm(accumulate(first, k) if k > 1 else first[0]) / np.float32(2))       # half the first update's norm
        a.set_clip(max_norm)
    for u, lr in enumerate(LRS):
        logical, padded = [], []
        for j, (x, y) in enumerate(batches):
            gdev, gpad = grad(b, x, y, p)
            logical.append(b.unpad(gdev))
            padded.append(gpad)
            step(a, x, y, lr)
            if k > 1:
                assert same_bits(a.get_accumulated(), accumulate(logical, k)), (u, j)
                assert j == k - 1 or same_bits(a.get_params(), p), (u, j)
        g, gpad = (accumulate(logical, k), accumulate(padded, k)) if k > 1 else (logical[0], padded[0])
        if clip:
            norm, coef = a.grad_norm()
            check_norm(f"update {u}", norm, coef, grad_norm(gpad), max_norm)
            assert u > 0 or coef < 1.0
            g = apply_coef(g, coef)
        if sgd:
            p, v = sgd_update(p, g, v, lr, *opt)
        else:
            p = plain_update(p, g, lr)
        if ema:
            e = ema_update(e, p, DECAY)
        assert same_bits(a.get_params(), p), (u, float(np.abs(a.get_params() - p).max()))
        assert same_bits(a.get_velocity(), v), u
        if ema:
            assert same_bits(a.get_ema(), e), u
    if clip:
        assert a.grad_norm_count() == len(LRS)
    a.close(); b.close()


@pytest.mark.parametrize("clip,sgd,ema,k", FORMS, ids=FORM_IDS)
def test_epoch_with_device_rate_is_the_batches_fed_one_by_one(clip, sgd, ema, k):
    """train_epoch over a resident uint8 set of four batches, the rate from a device tensor (the _dlr forms), against a twin fed the same
    batches by gather_batch + train_step at the same float rates"""
    import torch
    spec = PLAIN_HEAD
    in_shape, layers, B = spec
    a, t = twins(spec, "fp32")
    rng = np.random.default_rng(6)
    X = a.to_device(rng.integers(0, 256, (4 * B,) + in_shape).astype(np.uint8))
    Y = a.to_device(rng.integers(0, layers[-1][1], 4 * B).astype(np.int32))
    rates = np.array([0.01, 0.05, 0.03, 0.02], dtype=np.float32)
    lr = a.to_device(rates)
    a.synchronize()
    if clip:
        with torch.cuda.stream(t.stream):
            x0, y0 = t.gather_batch(X, Y, None, B)
        max_norm = float(grad_norm(grad(t, x0, y0)[1]) / np.float32(4))       # a quarter of the first batch's norm: it bites on a mean of two too
    for n in (a, t):
        _configure(n, sgd, ema, k)
        if clip:
            n.set_clip(max_norm)
    g0 = a.graphs_instantiated()
    with torch.cuda.stream(a.stream):
        a.train_epoch(X, Y, None, B, lr)
    a.synchronize()
    assert a.graphs_instantiated() == g0 + k             # one graph per B, or one per kind of micro-step (first, last) and B
    keep = []
    for s in range(4):
        with torch.cuda.stream(t.stream):
            x, y = t.gather_batch(X, Y, None, B, base=s * B)
            keep.append((x, y))
            t.train_step(x, y, float(rates[s]))
        t.synchronize()
        if clip and s == k - 1:
            assert t.grad_norm()[1] < 1.0                # clipping bites on the first update
    assert same_bits(a.get_params(), t.get_params()) and same_bits(a.get_velocity(), t.get_velocity())
    if ema:
        assert same_bits(a.get_ema(), t.get_ema())
    if k > 1:
        assert a.get_accumulate() == t.get_accumulate() == (k, 0) and same_bits(a.get_accumulated(), t.get_accumulated())
    if clip:
        assert a.grad_norm() == t.grad_norm() and a.grad_norm_count() == t.grad_norm_count() == 4 // k
    a.close(); t.close()


# ---- the plan text -----------------------------------------------------------------------------------------------------------------------
PLAN_LINES = ("  reduction:", "  gradient:", "  norm:", "  update:", "  graph:")
PLAN_CONFIGS = list(itertools.product([False, True], [False, True], [False, True], [1, 3]))        # (clip, sgd, ema, accumulate)
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "update_plans.json")


def _update_plans():
    """{configuration: {plan: its lines on the reduction, the norm, the update and the graph}} of a FUSED_HEAD net"""
    B = FUSED_HEAD[2]
    out = {}
    for clip, sgd, ema, k in PLAN_CONFIGS:
        net = make_net(FUSED_HEAD)
        _configure(net, sgd, ema, k)
        if clip:
            net.set_clip(1.0)
        plans = {"step": net.plan_of_this_net(B),
                 "epoch_host_rate": net.plan_epoch_of_this_net(B, lr_from_device=False),
                 "epoch_device_rate": net.plan_epoch_of_this_net(B, lr_from_device=True)}
        if k > 1:
            for kind in ("first", "middle", "last"):
                plans["micro_" + kind] = net.plan_micro_of_this_net(B, kind)
        net.close()
        out[f"clip{int(clip)}-sgd{int(sgd)}-ema{int(ema)}-acc{k}"] = {name: [ln for ln in text.splitlines() if ln.startswith(PLAN_LINES)] for name, text in plans.items()}
    return out


def test_plan_text_is_what_the_named_kernels_printed():
    with open(GOLDEN) as f:
        want = json.load(f)
    got = _update_plans()
    assert sorted(got) == sorted(want) and len(want) == len(PLAN_CONFIGS)
    for config in want:
        assert got[config] == want[config], config


if __name__ == "__main__":
    with open(sys.argv[1], "w") as f:
        json.dump(_update_plans(), f, indent=1, sort_keys=True)
        f.write("\n")
