"""GPU tests of Track X's label smoothing and mixup / CutMix on the epoch's one graph (include/rcn_hipx.h): rcn_hipx_set_loss and the
soft loss kernels (k_softmax_ce_soft, k_head_f32's soft instantiation), rcn_hipx_train_step_pair_dev, the mixing gather
(rcn_hipx_gather_mix_dev, k_gather_mix), rcn_hipx_train_epoch_mix_dev and rcn_hipx_plan_epoch_mix_net.

The gather moves and blends stored values with one rounding per operation, so it is held bit for bit against tests/_mix_ref.py; a mixed
epoch is held bit for bit against gather_mix + train_step_pair, and an epoch that mixes nothing against the un-mixed epoch.  The loss
and the gradients are held against the f64 restatement of tests/_mix_ref.py (pinned to the oracle and to finite differences by
tests/test_convnet_mix_plan.py) at the tolerances tests/test_gpu_convnet.py uses for the same comparisons: loss |d| <= 2e-4 max(1, loss);
gradients 2e-4 of scale for fp32 and 5e-3 for bf16 operands."""
import re

import numpy as np
import pytest
from _convnet_util import (CIFAR, FUSED_HEAD, KW, NESTEROV, ODD_WIDTH, PLAIN_HEAD, POOL_PAIRS, close, dev, epoch, make_net, mix_records, oracle_params, random_set, same_state, sync,
                           twins, widen, zeros)
from _mix_ref import gather_mix_ref, soft_loss_and_grads, soft_loss_f64, soft_targets

from oracle import convnet_oracle as co

pytestmark = pytest.mark.gpu

SMALL = [(FUSED_HEAD, "fp32", False), (PLAIN_HEAD, "bf16", True), (POOL_PAIRS, "bf16_stored", False)]      # (net, precision, momentum SGD)
SMALL_IDS = ["fused_head-fp32", "plain_head-bf16-sgd", "pool_pairs-bf16_stored"]
ORACLE_MODE = {"fp32": ("f64", False, 2e-4), "bf16": ("bf16", False, 5e-3), "bf16_stored": ("bf16", True, 5e-3)}      # (operand, stored, rtol)


# ---- 1. the mixing gather is the formula -----------------------------------------------------------------------------------------------

def _mix_cases(H, W):
    """(blend, weight, y0, y1, x0, x1): mixup, an interior box (with and without a blend around it), a box on two edges, the whole image,
    an empty box, an inverted box, a box with corners outside the image, and the record that mixes nothing"""
    return [(0.3, 0.3, 0, 0, 0, 0), (1.0, 0.5, 1, H - 1, 2, W - 2), (0.7, 0.5, 1, H - 1, 2, W - 2), (1.0, 0.5, 0, H // 2, W // 2, W), (1.0, 0.0, 0, H, 0, W),
            (0.6, 0.6, 3, 3, 1, W), (0.5, 0.5, H - 1, 1, 0, W), (1.0, 0.5, -3, H + 5, -2, W // 2), (0.25, 0.5, -(1 << 31), (1 << 31) - 1, W - 1, (1 << 31) - 1),
            (1.0, 1.0, 0, 0, 0, 0)]


# every small net with both sets, augmented and not; the workload shape (the 16-byte path at B = 512) once
GATHER_CASES = [(spec, B, u8, aug) for spec, B in ((ODD_WIDTH, 4), (FUSED_HEAD, 5), (POOL_PAIRS, 64)) for u8 in (False, True) for aug in (False, True)] + [(CIFAR, 512, True, True)]
GATHER_IDS = ["%dx%dx%d-b%d-%s-%s" % (s[0] + (B, "uint8" if u8 else "fp32", "augmented" if aug else "plain")) for s, B, u8, aug in GATHER_CASES]


@pytest.mark.parametrize("spec,B,u8,aug", GATHER_CASES, ids=GATHER_IDS)
def test_gather_mix_is_the_blend_and_the_box_of_the_two_gathered_rows_bit_for_bit(spec, B, u8, aug):
    from mercer_research_amd.convnet import Augment
    (H, W, _), _, _ = spec
    net = make_net(spec)
    n = 2 * B + 3
    X, y = random_set(net, spec, n, seed=41, u8=u8)
    Xh, yh = X.cpu().numpy(), y.cpu().numpy()
    idxh = np.random.default_rng(42).permutation(n).astype(np.int32)[:B]
    idx = dev(net, idxh)
    augment = Augment(2, True, 7, 3) if aug else None
    q0 = 3 * B
    recs, recs_dev = mix_records(net, _mix_cases(H, W))
    plain, yp = net.gather_batch(X, y, idx, B, augment=augment, q0=q0, **KW)
    net.synchronize()
    plain = plain.cpu().numpy()
    assert plain.tobytes() == gather_mix_ref(Xh[idxh], recs[-1].tolist(), widen, (2, True, 7, 3) if aug else None, q0).tobytes()
    seen = set()
    for k, rec in enumerate(recs):
        x, ya, yb = net.gather_mix(X, y, idx, B, recs_dev[k:k + 1], augment=augment, q0=q0, **KW)
        net.synchronize()
        want = gather_mix_ref(Xh[idxh], rec.tolist(), widen, (2, True, 7, 3) if aug else None, q0)
        got = x.cpu().numpy()
        assert np.array_equal(got, want) and got.tobytes() == want.tobytes(), (k, rec)
        assert np.array_equal(ya.cpu().numpy(), yh[idxh]) and np.array_equal(yb.cpu().numpy(), yh[idxh[::-1]]), k
        seen.add(want.tobytes())
    assert len(seen) >= len(recs) - 1                                # the records are not all the same picture
    assert got.tobytes() == plain.tobytes()                          # blend 1 with an empty box: gather_batch's bytes
    if B % 2:                                                        # the middle row of an odd batch partners itself: a box changes nothing there
        x, _, _ = net.gather_mix(X, y, idx, B, recs_dev[1:2], augment=augment, q0=q0, **KW)
        net.synchronize()
        assert np.array_equal(x.cpu().numpy()[B // 2], plain[B // 2])
    # rows in order, without labels
    x, ya, yb = net.gather_mix(X, None, None, B, recs_dev[0:1], base=2, augment=augment, q0=q0, **KW)
    net.synchronize()
    assert ya is None and yb is None
    assert np.array_equal(x.cpu().numpy(), gather_mix_ref(Xh[2:2 + B], recs[0].tolist(), widen, (2, True, 7, 3) if aug else None, q0))
    net.close()


# ---- 2. the loss value -----------------------------------------------------------------------------------------------------------------

def _pair_batch(net, spec, seed):
    in_shape, layers, B = spec
    rng = np.random.default_rng(seed)
    x = rng.standard_normal((B,) + in_shape).astype(np.float32)
    ya = rng.integers(0, layers[-1][1], B).astype(np.int32)
    yb = rng.integers(0, layers[-1][1], B).astype(np.int32)
    return x, ya, yb, dev(net, x), dev(net, ya), dev(net, yb)


@pytest.mark.parametrize("eps", [0.0, 0.1])
@pytest.mark.parametrize("spec,precision,sgd", SMALL, ids=SMALL_IDS)
def test_pair_step_reports_the_soft_loss_of_its_own_logits(spec, precision, sgd, eps):
    import torch
    net = make_net(spec, precision)
    net.init_params(2)
    if sgd:
        net.set_sgd(0.9, 5e-4, True)
    net.set_loss(eps)
    assert net.get_loss() == float(np.float32(eps))
    x, ya, yb, xd, yad, ybd = _pair_batch(net, spec, 51)
    w = dev(net, np.array([0.3], dtype=np.float32))
    loss = zeros(net, 1)
    p0 = net.get_params()
    with torch.cuda.stream(net.stream):
        logits = net.forward(xd)
        net.train_step_pair(xd, yad, ybd, w, 0.0, loss)
    net.synchronize()
    assert np.array_equal(net.get_params(), p0)                      # lr = 0
    want = soft_loss_f64(logits.cpu().numpy(), ya, yb, float(np.float32(0.3)), float(np.float32(eps)))
    got = float(loss.item())
    print("loss", got, "f64 formula", want)
    assert abs(got - want) <= 2e-4 * max(1.0, want), (got, want)
    net.close()


# ---- 3. gradients ----------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("spec,precision,sgd", SMALL, ids=SMALL_IDS)
def test_smoothed_gradients_match_the_restated_oracle(spec, precision, sgd):
    import torch
    in_shape, layers, B = spec
    operand, stored, rtol = ORACLE_MODE[precision]
    rng = np.random.default_rng(B + 7)
    net = make_net(spec, precision)
    _, _, flat, w32, b32 = oracle_params(rng, in_shape, layers)
    net.set_params(flat)
    net.set_loss(0.1)
    x = rng.standard_normal((B,) + in_shape).astype(np.float32)
    y = rng.integers(0, layers[-1][1], B).astype(np.int32)
    xd, yd = dev(net, x), dev(net, y)
    T = soft_targets(y, y, 1.0, float(np.float32(0.1)), layers[-1][1])
    loss_ref, _, gws, gbs = soft_loss_and_grads(x.astype(np.float64), T, w32, b32, layers, operand, stored)
    loss = zeros(net, 1)
    with torch.cuda.stream(net.stream):
        grad = net.gradients(xd, yd, loss=loss)
    net.synchronize()
    print("loss", loss.item(), "ref", loss_ref)
    assert abs(loss.item() - loss_ref) <= rtol * max(1.0, loss_ref)
    close(net.unpad(grad), co.flatten(gws, gbs), rtol=rtol)
    # the bucketed walk computes the same loss and gradients
    grad2 = torch.zeros_like(grad)
    loss2 = zeros(net, 1)                                           # (synchronises: grad2 is ready)
    with torch.cuda.stream(net.stream):
        net.gradients_bucketed(xd, yd, grad2, loss=loss2, min_bucket_bytes=0)
    net.synchronize()
    assert np.array_equal(grad2.cpu().numpy(), grad.cpu().numpy()) and loss2.item() == loss.item()
    net.close()


@pytest.mark.parametrize("precision", ["fp32", "bf16"])
@pytest.mark.parametrize("spec", [FUSED_HEAD, PLAIN_HEAD], ids=["fused_head", "plain_head"])
def test_pair_step_moves_the_parameters_by_the_restated_gradient(spec, precision):
    import torch
    in_shape, layers, B = spec
    operand, stored, rtol = ORACLE_MODE[precision]
    rng = np.random.default_rng(B + 9)
    net = make_net(spec, precision)
    _, _, flat, w32, b32 = oracle_params(rng, in_shape, layers)
    net.set_params(flat)
    net.set_loss(0.1)
    x, ya, yb, xd, yad, ybd = _pair_batch(net, spec, 61)
    w = dev(net, np.array([0.3], dtype=np.float32))
    T = soft_targets(ya, yb, float(np.float32(0.3)), float(np.float32(0.1)), layers[-1][1])
    _, _, gws, gbs = soft_loss_and_grads(x.astype(np.float64), T, w32, b32, layers, operand, stored)
    p0 = net.get_params()
    with torch.cuda.stream(net.stream):
        net.train_step_pair(xd, yad, ybd, w, 1.0)
    net.synchronize()
    close(p0.astype(np.float64) - net.get_params().astype(np.float64), co.flatten(gws, gbs), rtol=rtol)
    net.close()


# ---- 4. swap symmetry ------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("spec,precision,sgd", SMALL, ids=SMALL_IDS)
def test_swapping_the_pair_and_the_weight_changes_no_bit(spec, precision, sgd):
    import torch
    a, b = twins(spec, precision, sgd=NESTEROV if sgd else None)
    for net in (a, b):
        net.set_loss(0.1)
    x, ya, yb, xd, yad, ybd = _pair_batch(a, spec, 71)
    assert not np.array_equal(ya, yb)
    wa, wb = dev(a, np.array([0.25], dtype=np.float32)), dev(a, np.array([0.75], dtype=np.float32))
    la, lb = zeros(a, 1), zeros(a, 1)
    p0 = a.get_params()
    for _ in range(2):                                               # the eager step, then its graph
        with torch.cuda.stream(a.stream):
            a.train_step_pair(xd, yad, ybd, wa, 0.05, la)
        with torch.cuda.stream(b.stream):
            b.train_step_pair(xd, ybd, yad, wb, 0.05, lb)
        a.synchronize(); b.synchronize()
        assert la.cpu().numpy().tobytes() == lb.cpu().numpy().tobytes() and same_state(a, b)
    assert not np.array_equal(a.get_params(), p0) and np.isfinite(la.item())
    a.close(); b.close()


# ---- 5. a mixed epoch is its parts -----------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("spec,precision,sgd", SMALL, ids=SMALL_IDS)
def test_mixed_epoch_is_gather_mix_and_train_step_pair_bit_for_bit(spec, precision, sgd):
    import torch
    from mercer_research_amd.convnet import Augment, mix_plan
    (H, W, _), _, B = spec
    nb = 4
    a, b = twins(spec, precision, sgd=NESTEROV if sgd else None)
    for net in (a, b):
        net.set_loss(0.1)
    n = nb * B + 1
    X, y = random_set(a, spec, n, seed=81, u8=precision != "bf16")
    perm = dev(a, np.random.default_rng(82).permutation(n).astype(np.int32))
    rates = (0.002 * (1 + np.arange(nb))).astype(np.float32)
    lr = dev(a, rates)
    aug = Augment(2, True, 11, 0)
    rec = mix_plan(nb, H, W, mixup_alpha=0.8, cutmix_alpha=1.0, seed=5)
    rec[0] = (0.4, 0.4, 0, 0, 0, 0)                                  # whatever the draws are: one mixup step and one CutMix step
    rec[1] = (1.0, np.float32(1.0 - 6.0 / (H * W)), 1, 3, 2, 5)
    recs_dev = a.mix_to_device(rec)
    sync()
    # a plain epoch first: its graph must survive the mixed ones
    epoch(a, X, y, perm, B, lr, augment=aug, **KW)
    epoch(b, X, y, perm, B, lr, augment=aug, **KW)
    assert same_state(a, b)
    g_plain = a.graphs_instantiated()
    la = zeros(a, nb)
    epoch(a, X, y, perm, B, lr, losses=la, augment=aug, mix=recs_dev, **KW)
    g_mix = a.graphs_instantiated()
    assert g_mix - g_plain == 1
    lb = zeros(b, nb)
    keep = []
    with torch.cuda.stream(b.stream):
        for s in range(nb):
            x, ya, yb = b.gather_mix(X, y, perm[s * B:(s + 1) * B].contiguous(), B, recs_dev[s:s + 1], augment=aug, q0=s * B, **KW)
            w = torch.tensor([float(rec["weight"][s])], dtype=torch.float32, device=b.device)
            keep.append((x, ya, yb, w))
            b.train_step_pair(x, ya, yb, w, float(rates[s]), lb[s:s + 1])
    b.synchronize()
    assert np.array_equal(la.cpu().numpy(), lb.cpu().numpy()), (la.cpu().numpy(), lb.cpu().numpy())
    assert same_state(a, b)
    assert np.all(np.isfinite(lb.cpu().numpy())) and np.all(lb.cpu().numpy() > 0)
    # other records, another schedule: the same graph; and the plain epoch still replays its own
    rec2 = mix_plan(nb, H, W, cutmix_alpha=1.0, seed=6)
    lr2 = dev(a, (rates * np.float32(0.37)).astype(np.float32))
    epoch(a, X, y, perm, B, lr2, augment=aug, mix=a.mix_to_device(rec2), **KW)
    epoch(a, X, y, None, B, lr2[1:3].contiguous(), first_batch=1, n_batches=2, mix=a.mix_to_device(rec2[1:3]), **KW)
    assert a.graphs_instantiated() == g_mix
    epoch(a, X, y, perm, B, lr, augment=aug, **KW)
    assert a.graphs_instantiated() == g_mix
    a.close(); b.close()


# ---- 6. nothing configured changes nothing ---------------------------------------------------------------------------------------------

@pytest.mark.parametrize("spec,precision,sgd", SMALL, ids=SMALL_IDS)
def test_records_that_mix_nothing_give_the_unmixed_epoch_bit_for_bit(spec, precision, sgd):
    from mercer_research_amd.convnet import Augment
    B, nb = spec[2], 4
    a, b = twins(spec, precision, sgd=NESTEROV if sgd else None)
    assert a.get_loss() == 0.0
    n = nb * B + 2
    X, y = random_set(a, spec, n, seed=91, u8=precision != "bf16")
    perm = dev(a, np.random.default_rng(92).permutation(n).astype(np.int32))
    _, recs_dev = mix_records(a, [(1.0, 1.0, 0, 0, 0, 0)] * nb)
    la, lb = zeros(a, nb), zeros(b, nb)
    for lr, aug in ((0.03, None), (dev(a, (0.01 * (1 + np.arange(nb))).astype(np.float32)), Augment(1, True, 3, 0))):
        epoch(a, X, y, perm, B, lr, losses=la, augment=aug, mix=recs_dev, **KW)
        epoch(b, X, y, perm, B, lr, losses=lb, augment=aug, **KW)
        assert la.cpu().numpy().tobytes() == lb.cpu().numpy().tobytes(), (la.cpu().numpy(), lb.cpu().numpy())
        assert same_state(a, b)
    a.close(); b.close()


def test_a_loss_of_257_workgroups_is_the_restated_sum_of_its_rows_hard_and_soft():
    """B = 2049 on ODD_WIDTH (no fused head): 257 workgroups of 8 samples, the last with one, so "thread 0" of the last-arriving workgroup
    takes the partials of blocks 0 and 256.  The pair step at eps = 0, w = 1 gives the hard step's bits; and the step's loss is the
    float32 restatement, in the kernel's order, of the per-row losses evaluate_metrics returns for the same parameters and batch before
    the step (the row expression is the one routine of both kernels)."""
    import _eval_ref
    import torch
    B = 2049
    spec = (ODD_WIDTH[0], ODD_WIDTH[1], B)
    a, b = twins(spec, "fp32")
    assert "k_softmax_ce, 257 workgroups" in a.plan_of_this_net(B)
    x, ya, yb, xd, yad, ybd = _pair_batch(a, spec, 97)
    out = a.evaluate_metrics_async(xd, yad, topk=(1,), confusion=False, per_row=True)
    a.synchronize()
    each = out["loss_each"].cpu().numpy().copy()
    one = dev(b, np.array([1.0], dtype=np.float32))
    la, lb = zeros(a, 1), zeros(b, 1)
    with torch.cuda.stream(a.stream):
        a.train_step(xd, yad, 0.05, la)
    with torch.cuda.stream(b.stream):
        b.train_step_pair(xd, yad, ybd, one, 0.05, lb)
    a.synchronize(); b.synchronize()
    hard, soft, want = la.cpu().numpy(), lb.cpu().numpy(), _eval_ref.step_loss_from_rows(each)
    print(f"hard {hard[0]!r} soft {soft[0]!r} restated {want!r} float64 mean {float(each.astype(np.float64).mean())!r}")
    assert hard.tobytes() == soft.tobytes() and same_state(a, b)
    assert hard.tobytes() == want.tobytes(), (hard, want)
    a.close(); b.close()


# ---- 7. set_loss -----------------------------------------------------------------------------------------------------------------------

def test_set_loss_refusals_round_trip_evaluation_and_plans():
    import torch
    from mercer_research_amd.convnet import Augment
    soft = re.compile(r"k_softmax_ce_soft|k_head_f32<true, true>")
    for spec in (FUSED_HEAD, PLAIN_HEAD):
        B = spec[2]
        a, b = twins(spec, "fp32")
        X, y = random_set(a, spec, 3 * B, seed=95, u8=True)
        a.set_loss(0.25)
        for bad in (-0.1, 1.0, float("nan"), float("inf"), -float("inf")):
            assert a.lib.rcn_hipx_set_loss(a.net, bad) == -1 and b"set_loss" in a.lib.rcn_hipx_last_error(a.net)
            assert a.get_loss() == 0.25
        a.set_loss(0.0)
        e0 = a.evaluate(X, y, **KW)
        plan0 = a.plan_of_this_net(B)
        assert not soft.search(plan0) and "label smoothing" not in plan0 and plan0 == b.plan_of_this_net(B)
        a.set_loss(0.1)
        assert a.get_loss() == float(np.float32(0.1))
        plan1 = a.plan_of_this_net(B)
        assert len(soft.findall(plan1)) == 1 and "label smoothing 0.1" in plan1 and "pair labels" not in plan1
        assert [l for l in plan1.splitlines() if not soft.search(l)] == [l for l in plan0.splitlines() if "k_softmax_ce" not in l and "k_head_f32" not in l]
        assert a.evaluate(X, y, **KW) == e0                          # evaluation stays the plain cross-entropy
        # a smoothed step differs from a plain one ...
        x, ya, yb, xd, yad, ybd = _pair_batch(a, spec, 96)
        p0 = a.get_params()
        la, lb = zeros(a, 1), zeros(b, 1)
        with torch.cuda.stream(a.stream):
            a.train_step(xd, yad, 0.05, la)
        a.synchronize()
        smoothed = a.get_params()
        # ... and after set_loss(0) the net steps as one never configured
        a.set_params(p0)
        a.set_loss(0.0)
        assert a.plan_of_this_net(B) == plan0
        for _ in range(2):
            with torch.cuda.stream(a.stream):
                a.train_step(xd, yad, 0.05, la)
            with torch.cuda.stream(b.stream):
                b.train_step(xd, yad, 0.05, lb)
            a.synchronize(); b.synchronize()
            assert np.array_equal(a.get_params(), b.get_params()) and la.cpu().numpy().tobytes() == lb.cpu().numpy().tobytes()
        assert not np.array_equal(smoothed, p0)
        b.set_params(p0)
        with torch.cuda.stream(b.stream):
            b.train_step(xd, yad, 0.05, lb)
        b.synchronize()
        assert not np.array_equal(b.get_params(), smoothed)
        # the mixed epoch's plan: the gather, the weight copy, the pair graph key, the soft loss
        lines = lambda text: [l.strip() for l in text.splitlines() if l.strip()]
        for sched in (False, True):
            for aug in (None, Augment(2, True, 1, 0)):
                plain = lines(a.plan_epoch_of_this_net(B, "uint8", sched, aug))
                got = lines(a.plan_epoch_of_this_net(B, "uint8", sched, aug, mix=True))
                assert got[1].startswith("gather: k_gather_mix<uint8, ") and "partner row B - 1 - r" in got[1]
                assert got[1].endswith("augment pad 2 hflip 1" if aug else "no augmentation")
                at = got.index(plain[plain.index(next(l for l in plain if l.startswith("graph: "))) + 1])
                head = got[2:at]
                assert [l.split(":")[0] for l in head] == (["lr"] if sched else []) + ["weight", "graph"]
                assert head[-2].startswith("weight: 4-byte device copy of mix_dev[i].weight")
                assert head[-1] == ("graph: one graph per B, lr from device, pair labels" if sched else "graph: one graph per (B, lr), pair labels")
                body = got[at:]
                assert sum(bool(soft.search(l)) for l in body) == 1 and any("label smoothing 0, pair labels" in l for l in body)
                assert a.plan_epoch_of_this_net(B, "uint8", sched, aug, mix=False) == a.plan_epoch_of_this_net(B, "uint8", sched, aug)
        a.close(); b.close()
    # the 16-byte and the scalar path of the mixing gather, as the plan names them
    c = make_net(CIFAR)
    assert "k_gather_mix<uint8, 4>, one or two source elements per output, 16-byte stores, 1536 workgroups" in c.plan_epoch_of_this_net(512, "uint8", mix=True)
    c.close()
    o = make_net(ODD_WIDTH)
    assert "k_gather_mix<float, 1>, element by element, 1 workgroups" in o.plan_epoch_of_this_net(4, "float32", mix=True)
    o.close()
