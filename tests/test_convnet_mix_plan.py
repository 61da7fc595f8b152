"""CPU tests of Track X's label smoothing and mixup / CutMix pieces that need no GPU (include/rcn_hipx.h: rcn_hipx_set_loss,
rcn_hipx_mix_step): the record's layout, mix_plan's draws, the refusals of the new entry points, and the two pins of the host
restatement the GPU comparisons rest on (tests/_mix_ref.py) -- bit for bit against oracle/convnet_oracle.py for a one-hot target, and
against central finite differences for a soft one."""
import ctypes as C

import numpy as np
import pytest
from _convnet_util import FUSED_HEAD, PLAIN_HEAD, convnet_loaded, oracle_params  # noqa: F401  (convnet_loaded: the fixture `convnet`)
from _mix_ref import soft_loss_and_grads, soft_loss_f64, soft_targets

from oracle import convnet_oracle as co


def test_mix_step_is_the_headers_24_bytes(convnet):
    assert C.sizeof(convnet.MixStep) == 24 and convnet.MIX_DTYPE.itemsize == 24
    for name, _ in convnet.MixStep._fields_:
        assert getattr(convnet.MixStep, name).offset == convnet.MIX_DTYPE.fields[name][1], name
    assert [n for n, _ in convnet.MixStep._fields_] == list(convnet.MIX_DTYPE.names) == ["blend", "weight", "y0", "y1", "x0", "x1"]
    rec = np.zeros(1, dtype=convnet.MIX_DTYPE)
    rec[0] = (0.25, 0.75, 1, 2, 3, 4)
    s = convnet.MixStep.from_buffer_copy(rec.tobytes())
    assert (s.blend, s.weight, s.y0, s.y1, s.x0, s.x1) == (0.25, 0.75, 1, 2, 3, 4)


@pytest.mark.parametrize("H,W", [(32, 32), (5, 7)])
def test_mix_plan_invariants(convnet, H, W):
    n = 2000
    for kw in (dict(mixup_alpha=0.8, cutmix_alpha=1.0), dict(mixup_alpha=0.2), dict(cutmix_alpha=1.0), dict(mixup_alpha=1.0, cutmix_alpha=0.5, switch_prob=0.9)):
        p = convnet.mix_plan(n, H, W, seed=3, **kw)
        assert p.dtype == convnet.MIX_DTYPE and p.shape == (n,)
        assert p.tobytes() == convnet.mix_plan(n, H, W, seed=3, **kw).tobytes()          # the same seed: the same bytes
        assert p.tobytes() != convnet.mix_plan(n, H, W, seed=4, **kw).tobytes()
        # boxes lie inside the image
        assert np.all((0 <= p["y0"]) & (p["y0"] <= p["y1"]) & (p["y1"] <= H) & (0 <= p["x0"]) & (p["x0"] <= p["x1"]) & (p["x1"] <= W))
        area = (p["y1"] - p["y0"]).astype(np.int64) * (p["x1"] - p["x0"])
        cut = p["blend"] == np.float32(1.0)                                               # (a mixup row with lam == 1.0f would also mix nothing)
        mixup = ~cut
        assert np.array_equal(p["weight"][cut & (area > 0)], (1.0 - area[cut & (area > 0)] / (H * W)).astype(np.float32))
        assert np.all(p["weight"][cut & (area == 0)] == np.float32(1.0))
        assert np.all(area[mixup] == 0) and np.array_equal(p["blend"][mixup], p["weight"][mixup])
        assert np.all((p["blend"][mixup] >= 0) & (p["blend"][mixup] <= 1))
        both = kw.get("mixup_alpha", 0) > 0 and kw.get("cutmix_alpha", 0) > 0
        if both:
            frac = np.mean(area > 0)
            assert 0.2 < frac <= 1.0 and mixup.any() and (area > 0).any()
        elif kw.get("cutmix_alpha", 0) > 0:
            assert cut.all() and (area > 0).any()
        else:
            assert np.all(area == 0) and mixup.sum() > n * 0.9
    for bad in (dict(mixup_alpha=-0.1, cutmix_alpha=1.0), dict(mixup_alpha=1.0, cutmix_alpha=-1.0), dict(), dict(mixup_alpha=0.0, cutmix_alpha=0.0)):
        with pytest.raises(ValueError):
            convnet.mix_plan(4, H, W, **bad)
    for bad_n in (0, -3):
        with pytest.raises(ValueError):
            convnet.mix_plan(bad_n, H, W, mixup_alpha=1.0)


def test_new_entry_points_refuse_null_nets_and_touch_nothing(convnet):
    lib = convnet.load()
    eps = C.c_float(9.0)
    assert lib.rcn_hipx_set_loss(None, 0.1) == -1
    assert lib.rcn_hipx_get_loss(None, C.byref(eps)) == -1 and eps.value == 9.0
    assert lib.rcn_hipx_train_step_pair_dev(None, None, None, None, None, 1, 0.1, None) == -1
    a = convnet.AugmentStruct(2, 1, 0, 0)
    assert lib.rcn_hipx_gather_mix_dev(None, None, 0, 1.0, 0.0, None, 1, None, 0, 1, C.byref(a), 0, None, None, None, None) == -1
    assert lib.rcn_hipx_train_epoch_mix_dev(None, None, 0, 1.0, 0.0, None, 1, None, 1, 0, 1, 0.1, None, C.byref(a), None, None) == -1
    buf = C.create_string_buffer(b"untouched", 64)
    assert lib.rcn_hipx_plan_epoch_mix_net(None, 1, 0, 0, None, 1, buf, len(buf)) == -1 and buf.value == b"untouched"
    assert lib.rcn_hipx_plan_epoch_mix_net(None, 1, 1, 1, C.byref(a), 0, buf, len(buf)) == -1 and buf.value == b"untouched"


@pytest.mark.parametrize("operand,stored", [("f64", False), ("bf16", False), ("bf16", True)], ids=["f64", "bf16", "bf16_stored"])
@pytest.mark.parametrize("spec", [FUSED_HEAD, PLAIN_HEAD], ids=["fused_head", "plain_head"])
def test_restatement_with_a_one_hot_target_is_the_oracle_bit_for_bit(spec, operand, stored):
    in_shape, layers, B = spec
    rng = np.random.default_rng(11)
    ws, bs = oracle_params(rng, in_shape, layers)[:2]
    x = rng.standard_normal((B,) + in_shape)
    y = rng.integers(0, layers[-1][1], B)
    want = co.loss_and_grads(x, y, ws, bs, layers, operand, stored)
    got = soft_loss_and_grads(x, soft_targets(y, y, 1.0, 0.0, layers[-1][1]), ws, bs, layers, operand, stored)
    assert got[0] == want[0] and np.array_equal(got[1], want[1])
    for i in range(len(ws)):
        assert np.array_equal(got[2][i], want[2][i]) and np.array_equal(got[3][i], want[3][i]), i


def test_soft_loss_gradients_match_finite_differences():
    """tests/test_convnet_oracle.py's net, step (1e-6) and tolerance (1e-6 * max(1, |num|)) on the loss against a soft target:
    eps = 0.1, two labels, w = 0.3."""
    layers = (("conv", 4), ("pool",), ("conv", 6), ("pool",), ("dense_relu", 8), ("dense", 5))
    in_shape = (8, 8, 3)
    rng = np.random.default_rng(0)
    x = rng.standard_normal((3,) + in_shape)
    ya, yb = rng.integers(0, 5, 3), rng.integers(0, 5, 3)
    T = soft_targets(ya, yb, 0.3, 0.1, 5)
    assert np.allclose(T.sum(axis=1), 1.0) and T.min() >= 0.02 - 1e-12
    ws = [rng.standard_normal(k) * 0.3 for k, _ in co.param_shapes(in_shape, layers)]
    bs = [rng.standard_normal(n) * 0.1 for _, n in co.param_shapes(in_shape, layers)]
    loss, logits, gws, gbs = soft_loss_and_grads(x, T, ws, bs, layers)
    assert abs(loss - soft_loss_f64(logits, ya, yb, 0.3, 0.1)) <= 1e-12 * max(1.0, loss)      # the dense form is the header's formula
    step = 1e-6

    def numeric(arr, idx):
        old = arr[idx]
        arr[idx] = old + step; lp = soft_loss_and_grads(x, T, ws, bs, layers)[0]
        arr[idx] = old - step; lm = soft_loss_and_grads(x, T, ws, bs, layers)[0]
        arr[idx] = old
        return (lp - lm) / (2 * step)

    checked = 0
    for li in range(len(ws)):
        for _ in range(2):
            idx = tuple(rng.integers(0, s) for s in ws[li].shape)
            num = numeric(ws[li], idx)
            assert abs(num - gws[li][idx]) <= 1e-6 * max(1.0, abs(num)), (li, idx, num, gws[li][idx])
            checked += 1
        j = int(rng.integers(0, bs[li].size))
        num = numeric(bs[li], j)
        assert abs(num - gbs[li][j]) <= 1e-6 * max(1.0, abs(num)), (li, j, num, gbs[li][j])
        checked += 1
    assert checked == 12
