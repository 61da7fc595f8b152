"""CPU checks of Track-X gradient clipping by global norm (include/rcn_hipx.h, rcn_hipx_set_clip): the NumPy restatement the GPU tests
compare with (tests/_clip_ref.py) is torch.nn.utils.clip_grad_norm_ on float64 tensors, its edge cases, and the new entry points exist, are
bound and refuse a null net without a GPU."""
import ctypes as C
import re

import numpy as np
import pytest
from _clip_ref import apply_coef, clip, clip_coef, grad_norm, grad_sumsq, plain_update
from _convnet_util import HEADER, libx  # noqa: F401  (libx: a fixture)

NEW = ["rcn_hipx_set_clip", "rcn_hipx_get_clip", "rcn_hipx_get_grad_norm", "rcn_hipx_set_grad_norm_log", "rcn_hipx_get_grad_norm_count", "rcn_hipx_grad_norm_dev"]
SIZES = [864, 32, 18432, 64, 73728, 128, 524288, 256, 2208]      # several tensors, 620 000 elements in all
assert sum(SIZES) == 620000


@pytest.fixture(scope="module")
def grads():
    rng = np.random.default_rng(11)
    return [(rng.standard_normal(n) * s).astype(np.float32) for n, s in zip(SIZES, [1.0, 0.1, 3e-2, 1.0, 1e-2, 0.5, 4e-3, 2.0, 1e-3])]


@pytest.mark.parametrize("max_norm,bites", [(1.0, True), (0.25, True), (1e-3, True), (1e6, False), (float("inf"), False)])
def test_restatement_is_torch_clip_grad_norm_on_float64(grads, max_norm, bites):
    """norm within 2^-23 relative (one float rounding of the exact root, doubled), coefficient within 2.5e-7 relative (three float
    roundings), clipped gradients fl(coef * g) bit for bit -- and within the coefficient's bound plus one rounding of torch's own."""
    import torch
    params = [torch.zeros(g.size, dtype=torch.float64, requires_grad=True) for g in grads]
    for q, g in zip(params, grads):
        q.grad = torch.from_numpy(g.astype(np.float64))
    total = float(torch.nn.utils.clip_grad_norm_(params, max_norm, norm_type=2, error_if_nonfinite=False))
    flat = np.concatenate(grads)
    clipped, norm, coef = clip(flat, max_norm)
    assert norm.dtype == np.float32 and coef.dtype == np.float32 and clipped.dtype == np.float32
    assert abs(float(norm) - total) <= 2.0 ** -23 * total, (float(norm), total)
    tcoef = min(1.0, max_norm / (total + 1e-6))
    assert abs(float(coef) - tcoef) <= 2.5e-7 * tcoef, (float(coef), tcoef)
    assert (coef < 1) == bites and (bites or coef == np.float32(1))
    assert np.array_equal(clipped, np.float32(coef) * flat)
    assert np.array_equal(clipped, flat) == (not bites)
    ref = np.concatenate([q.grad.numpy() for q in params])
    assert np.all(np.abs(clipped.astype(np.float64) - ref) <= ((1 + 2.5e-7) * (1 + 2.0 ** -24) - 1) * np.abs(ref))


def test_scale_is_applied_first_and_rounded_once():
    rng = np.random.default_rng(2)
    g = rng.standard_normal(4100).astype(np.float32)
    x = (np.float32(0.3) * g).astype(np.float32)
    assert grad_sumsq(g, 0.3) == grad_sumsq(x) and grad_norm(g, 0.3) == grad_norm(x)
    gp, norm, coef = clip(g, 1.0, scale=0.3)
    assert coef < 1 and np.array_equal(gp, np.float32(coef) * x) and np.array_equal(gp, apply_coef(g, coef, 0.3))


def test_edge_cases():
    rng = np.random.default_rng(3)
    g = rng.standard_normal(4096 + 8).astype(np.float32)
    gp, norm, coef = clip(g, float("inf"))
    assert coef == np.float32(1) and np.array_equal(gp.view(np.uint32), g.view(np.uint32))
    gp, norm, coef = clip(np.zeros(64, dtype=np.float32), 0.5)
    assert norm == 0 and coef == np.float32(1) and not gp.any()
    bad = g.copy()
    bad[777] = np.nan
    gp, norm, coef = clip(bad, 1.0)
    assert np.isnan(norm) and np.isnan(coef) and np.isnan(gp).all()
    assert np.isnan(clip_coef(np.float32(np.inf), np.inf)) and clip_coef(np.float32(np.inf), 2.0) == 0
    assert clip_coef(np.float32(3.0), 1.5) == np.float32(1.5) / (np.float32(3.0) + np.float32(1e-6))
    assert grad_sumsq(np.zeros(0, dtype=np.float32)) == 0 and grad_norm(np.zeros(0, dtype=np.float32)) == 0


@pytest.mark.parametrize("n", [4, 4100, 4096 * 1030])
def test_norm_is_the_f64_norm_rounded(n):
    """4 and 4100: the short last block; 4096 * 1030: more than 1024 partials, the strided accumulation.  Within 2^-24 relative of the
    exact norm: the double sum's error is far below a float rounding."""
    rng = np.random.default_rng(n)
    g = (rng.standard_normal(n) * 0.7).astype(np.float32)
    exact = float(np.sqrt(np.sum(g.astype(np.float64) ** 2)))
    assert abs(float(grad_norm(g)) - exact) <= 2.0 ** -24 * exact
    if n == 4:
        x = g.astype(np.float64)
        assert grad_sumsq(g) == (x[0] * x[0] + x[1] * x[1]) + (x[2] * x[2] + x[3] * x[3])
    if n == 4100:
        # element 4096 .. 4099 are thread 0 of block 1: its partial is their s_t alone
        x = g[4096:].astype(np.float64)
        assert grad_sumsq(g) == grad_sumsq(g[:4096]) + ((x[0] * x[0] + x[1] * x[1]) + (x[2] * x[2] + x[3] * x[3]))


def test_plain_update_rounds_once():
    """p - lr g with one rounding, against exact rational arithmetic; it differs from the twice-rounded line somewhere on a longer vector"""
    from fractions import Fraction
    rng = np.random.default_rng(4)
    p, g = rng.standard_normal(3000).astype(np.float32), rng.standard_normal(3000).astype(np.float32)
    p[:3], g[:3] = (1.0, 1.0, 0.0), (2.0 ** -24, 2.0 ** -25, 0.0)        # an exact tie, a value below it, a padding element
    lr = np.float32(0.05)
    got = plain_update(p, g, lr)
    assert got.dtype == np.float32 and got[2] == 0
    for i in range(200):
        exact = Fraction(float(p[i])) - Fraction(float(lr)) * Fraction(float(g[i]))
        for c in (np.nextafter(got[i], np.float32(-np.inf)), np.nextafter(got[i], np.float32(np.inf))):
            assert abs(Fraction(float(got[i])) - exact) <= abs(Fraction(float(c)) - exact), i
    assert plain_update(np.float32([1.0]), np.float32([-2.0 ** -24]), 1.0)[0] == np.float32(1.0)     # an exact tie goes to the even neighbour
    # 2^30 + 128 + (64 - 2^-40): the float64 sum rounds to the half-way point and from there to the even neighbour above; one rounding stays below
    big = np.float32([2.0 ** 30 + 128.0])
    assert plain_update(big, np.float32([-(64.0 - 2.0 ** -17)]), np.float32(1 + 2.0 ** -23))[0] == big[0]
    assert not np.array_equal(got, p - lr * g)


def test_null_net_is_refused_without_a_gpu(libx):
    a, b = C.c_float(9.0), C.c_float(7.0)
    cnt = C.c_int64(5)
    for m in (0.0, 1.0, float("inf"), float("nan"), -1.0):
        assert libx.rcn_hipx_set_clip(None, m) == -1
    assert libx.rcn_hipx_get_clip(None, C.byref(a)) == -1 and a.value == 9.0
    assert libx.rcn_hipx_get_grad_norm(None, C.byref(a), C.byref(b)) == -1 and (a.value, b.value) == (9.0, 7.0)
    assert libx.rcn_hipx_set_grad_norm_log(None, C.c_void_p(16), 4) == -1
    assert libx.rcn_hipx_set_grad_norm_log(None, None, 0) == -1
    assert libx.rcn_hipx_get_grad_norm_count(None, C.byref(cnt)) == -1 and cnt.value == 5
    assert libx.rcn_hipx_grad_norm_dev(None, C.c_void_p(16), 4, 1.0, C.c_void_p(32)) == -1


def test_header_declares_the_entries_and_the_binding_table_has_them(libx):
    from mercer_research_amd import convnet
    raw_text = open(HEADER).read()
    text = re.sub(r"/\*.*?\*/", "", raw_text, flags=re.S)
    declared = set(re.findall(r"\b(rcn_hipx_[a-z0-9_]+)\s*\(", text))
    raw = C.CDLL(convnet.LIBX_PATH)
    for name in NEW:
        assert name in declared and name in convnet.SIGNATURES and hasattr(raw, name), name
    for method in ("set_clip", "get_clip", "grad_norm", "set_grad_norm_log", "grad_norm_count", "grad_norm_of"):
        assert callable(getattr(convnet.ConvNet, method)), method
    assert convnet.SIGNATURES["rcn_hipx_set_clip"][1] == convnet.SIGNATURES["rcn_hipx_set_ema"][1]
    assert convnet.SIGNATURES["rcn_hipx_grad_norm_dev"][1] == [C.c_void_p, C.c_void_p, C.c_int64, C.c_float, C.c_void_p]
