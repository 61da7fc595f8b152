"""CPU checks of Track-X gradient accumulation (include/rcn_hipx.h, rcn_hipx_set_accumulate): what is accumulated is the gradient of each
equal micro-batch's MEAN loss scaled by 1 / k (the f64 oracle's identity with the concatenated batch), the NumPy restatement the GPU tests
compare with (tests/_accum_ref.py) and its edge cases, and the new entry points exist, are bound and refuse a null net without a GPU."""
import ctypes as C
import re

import numpy as np
import pytest
from _accum_ref import accumulate, scale_of
from _convnet_util import FUSED_HEAD, HEADER, libx  # noqa: F401  (libx: a fixture)

from oracle import convnet_oracle as co

NEW = ["rcn_hipx_set_accumulate", "rcn_hipx_get_accumulate", "rcn_hipx_reset_accumulation", "rcn_hipx_get_accumulated", "rcn_hipx_plan_micro_net"]


@pytest.mark.parametrize("k", [2, 3])
def test_mean_of_micro_batch_gradients_is_the_gradient_of_the_concatenated_batch(k):
    """(1 / k) sum_j grad(batch_j) == grad(all k B rows) in f64 to 1e-12 relative: equal micro-batches, and the mean loss of each."""
    in_shape, layers, B = FUSED_HEAD
    rng = np.random.default_rng(k)
    shapes = co.param_shapes(in_shape, layers)
    ws = [rng.standard_normal(s) * np.sqrt(2.0 / s[0]) for s, _ in shapes]
    bs = [rng.standard_normal(n) * 0.1 for _, n in shapes]
    x = rng.standard_normal((k * B,) + in_shape)
    y = rng.integers(0, layers[-1][1], k * B).astype(np.int32)
    loss_all, _, gws, gbs = co.loss_and_grads(x, y, ws, bs, layers)
    whole = co.flatten(gws, gbs)
    parts, losses = [], []
    for j in range(k):
        l, _, gw, gb = co.loss_and_grads(x[j * B:(j + 1) * B], y[j * B:(j + 1) * B], ws, bs, layers)
        parts.append(co.flatten(gw, gb))
        losses.append(l)
    mean = sum(parts) / k
    scale = float(np.abs(whole).max())
    assert scale > 0 and float(np.abs(mean - whole).max()) <= 1e-12 * scale
    assert abs(sum(losses) / k - loss_all) <= 1e-12 * abs(loss_all)
    assert float(np.abs(sum(parts) - whole).max()) > 1e-3 * scale      # (the unscaled sum is NOT it)


def test_k_1_returns_the_gradient_unchanged():
    rng = np.random.default_rng(1)
    g = rng.standard_normal(4100).astype(np.float32)
    g[7] = -0.0
    got = accumulate([g], 1)
    assert got.dtype == np.float32 and np.array_equal(got.view(np.uint32), g.view(np.uint32))
    assert np.signbit(got[7]) and got[7] == 0                           # a -0.0 survives the store
    assert scale_of(1) == np.float32(1)


def test_the_scale_goes_in_per_micro_batch_not_at_the_end():
    """k = 3: fl(fl(fl(c g0) + fl(c g1)) + fl(c g2)) differs somewhere from fl(c * fl(fl(g0 + g1) + g2)); c = fl(1 / 3) is not a power of two"""
    rng = np.random.default_rng(5)
    g = [rng.standard_normal(4096).astype(np.float32) for _ in range(3)]
    c = scale_of(3)
    assert c == np.float32(1.0) / np.float32(3.0) and c.dtype == np.float32
    got = accumulate(g, 3)
    by_hand = ((c * g[0]) + (c * g[1])) + (c * g[2])
    assert by_hand.dtype == np.float32 and np.array_equal(got.view(np.uint32), by_hand.view(np.uint32))
    at_the_end = c * ((g[0] + g[1]) + g[2])
    assert not np.array_equal(got.view(np.uint32), at_the_end.view(np.uint32))
    assert float(np.abs(got - at_the_end).max()) <= 4 * 2.0 ** -24 * float(np.abs(at_the_end).max() + np.abs(np.stack(g)).max())
    # an open cycle holds the prefix
    assert np.array_equal(accumulate(g[:2], 3), (c * g[0]) + (c * g[1])) and np.array_equal(accumulate(g[:1], 3), c * g[0])
    # k = 2: c = 0.5 is exact, so only the sum rounds
    assert np.array_equal(accumulate(g[:2], 2), (np.float32(0.5) * g[0]) + (np.float32(0.5) * g[1]))


def test_null_net_is_refused_without_a_gpu(libx):
    k, pending = C.c_int(9), C.c_int(7)
    for v in (0, 1, 2, 65536, 65537, -1):
        assert libx.rcn_hipx_set_accumulate(None, v) == -1
    assert libx.rcn_hipx_get_accumulate(None, C.byref(k), C.byref(pending)) == -1 and (k.value, pending.value) == (9, 7)
    assert libx.rcn_hipx_reset_accumulation(None) == -1
    flat = np.full(8, 3.0, dtype=np.float32)
    assert libx.rcn_hipx_get_accumulated(None, flat.ctypes.data_as(C.POINTER(C.c_float))) == -1 and (flat == 3.0).all()
    buf = C.create_string_buffer(b"untouched", 64)
    for kind in (0, 1, 2, 3):
        assert libx.rcn_hipx_plan_micro_net(None, 4, kind, buf, len(buf)) == -1 and buf.value == b"untouched"


def test_header_declares_the_entries_and_the_binding_table_has_them(libx):
    from mercer_research_amd import convnet
    raw_text = open(HEADER).read()
    text = re.sub(r"/\*.*?\*/", "", raw_text, flags=re.S)
    declared = set(re.findall(r"\b(rcn_hipx_[a-z0-9_]+)\s*\(", text))
    raw = C.CDLL(convnet.LIBX_PATH)
    for name in NEW:
        assert name in declared and name in convnet.SIGNATURES and hasattr(raw, name), name
    for method in ("set_accumulate", "get_accumulate", "reset_accumulation", "get_accumulated", "plan_micro_of_this_net"):
        assert callable(getattr(convnet.ConvNet, method)), method
    assert convnet.SIGNATURES["rcn_hipx_set_accumulate"][1] == [C.c_void_p, C.c_int]
    assert convnet.SIGNATURES["rcn_hipx_get_accumulated"][1] == convnet.SIGNATURES["rcn_hipx_get_ema_params"][1]
    assert convnet.SIGNATURES["rcn_hipx_plan_micro_net"][1] == [C.c_void_p, C.c_int, C.c_int, C.c_char_p, C.c_int]
    assert "per micro-batch" in convnet.ConvNet.train_epoch.__doc__ and "np.repeat(schedule, k)" in convnet.ConvNet.train_epoch.__doc__
