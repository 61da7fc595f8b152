"""CPU checks of Track X's Adam and AdamW (include/rcn_hipx.h, rcn_hipx_set_adam): the NumPy restatement the GPU tests compare with is
torch.optim.Adam's / torch.optim.AdamW's update, it rounds every operation once on float32 arrays, and the new entry points exist, are
bound and refuse a null net without a GPU."""
import ctypes as C
import re

import numpy as np
import pytest
from _adam_ref import TICK0, adam_tick, adam_ticks, adam_update
from _convnet_util import HEADER, libx  # noqa: F401  (libx: a fixture)

NEW = ["rcn_hipx_set_adam", "rcn_hipx_get_adam", "rcn_hipx_get_adam_state", "rcn_hipx_set_adam_state", "rcn_hipx_reset_adam"]
B1, B2 = float(np.float32(0.9)), float(np.float32(0.999))      # the float32-rounded betas, as the library holds them


@pytest.mark.parametrize("weight_decay", [0.0, 5e-2])
@pytest.mark.parametrize("decoupled", [False, True], ids=["adam", "adamw"])
def test_restatement_is_torch_adam(decoupled, weight_decay):
    """float64 arrays against torch on float64, 20 steps: max |dp| <= 1e-12 (float64 rounding only: measured 6.7e-16 .. 1.3e-15 at
    max |p| of about 3.9)"""
    import torch
    rng = np.random.default_rng(3)
    n, lr, eps = 4096, 1e-3, 1e-8
    p0 = rng.standard_normal(n)
    tp = torch.tensor(p0, dtype=torch.float64, requires_grad=True)
    make = torch.optim.AdamW if decoupled else torch.optim.Adam
    opt = make([tp], lr=lr, betas=(B1, B2), eps=eps, weight_decay=weight_decay, amsgrad=False)
    p, m, v, state = p0.copy(), np.zeros(n), np.zeros(n), TICK0
    for _ in range(20):
        g = rng.standard_normal(n) * 10.0 ** rng.integers(-6, 1, n)
        g[::7] = 0.0
        tp.grad = torch.tensor(g, dtype=torch.float64)
        opt.step()
        state, c1, c2 = adam_tick(state, B1, B2, dtype=np.float64)
        p, m, v = adam_update(p, g, m, v, lr, c1, c2, B1, B2, eps, weight_decay, decoupled)
        ref = tp.detach().numpy()
        print("max |dp| =", float(np.abs(p - ref).max()), "max |p| =", float(np.abs(ref).max()))
        assert np.abs(p - ref).max() <= 1e-12
    assert p.dtype == np.float64 and state[0] == 20
    assert np.abs(m - opt.state[tp]["exp_avg"].numpy()).max() <= 1e-12 and np.abs(v - opt.state[tp]["exp_avg_sq"].numpy()).max() <= 1e-12


def _r32(x64):
    """float64 -> float32, one rounding"""
    return np.asarray(x64, dtype=np.float64).astype(np.float32)


def test_restatement_rounds_every_operation_in_float32():
    f = np.float32
    rng = np.random.default_rng(11)
    n = 512
    p, g = rng.standard_normal(n).astype(f), rng.standard_normal(n).astype(f)
    m, v = (rng.standard_normal(n) * 0.1).astype(f), (rng.random(n) * 0.1).astype(f)
    lr, eps, wd = f(0.1), f(1e-8), f(5e-2)                # a rate at which the update reaches the low bits of most parameters
    b1, b2 = f(0.9), f(0.999)
    a1, a2 = f(1) - b1, f(1) - b2
    (_, b1t, b2t), c1, c2 = adam_ticks(3, b1, b2)
    assert c1.dtype == f and c2.dtype == f

    # L2 form, step by step
    np_, nm, nv = adam_update(p, g, m, v, lr, c1, c2, b1, b2, eps, wd, False)
    assert np_.dtype == f and nm.dtype == f and nv.dtype == f
    x = g + wd * p
    diff = x - m
    mm = m + a1 * diff
    vv = b2 * v + a2 * (x * x)
    d = np.sqrt(vv) / c2 + eps
    step, quot = lr / c1, mm / d
    assert np.array_equal(nm, mm) and np.array_equal(nv, vv) and np.array_equal(np_, p - step * quot)
    # a1 * (x - m) is not fused into the sum: the fused form (the product exact in float64, one rounding of the sum) differs somewhere
    fused_m = _r32(m.astype(np.float64) + np.float64(a1) * diff.astype(np.float64))
    assert (fused_m != mm).any() and np.array_equal(mm, m + _r32(np.float64(a1) * diff.astype(np.float64)))
    # (lr / c1) * (m / d) is two roundings and a product, then the difference rounds: neither lr * m / (c1 * d) nor a fused subtract
    prod = step * quot
    assert np.array_equal(prod, _r32(np.float64(step) * quot.astype(np.float64)))
    other = p - (lr * mm) / (c1 * d)
    fused_p = _r32(p.astype(np.float64) - np.float64(step) * quot.astype(np.float64))
    assert (other != np_).any() and (fused_p != np_).any()

    # decoupled: p scaled by fl(1 - fl(lr * wd)) first, the gradient untouched
    lr2, wd2 = f(0.3), f(0.1)                            # fl(lr * wd) is inexact: 1 - lr * wd rounded once is another float32
    factor = f(1) - lr2 * wd2
    assert factor != _r32(1.0 - np.float64(lr2) * np.float64(wd2))
    wp, wm, wv = adam_update(p, g, m, v, lr2, c1, c2, b1, b2, eps, wd2, True)
    pm = m + a1 * (g - m)
    pv = b2 * v + a2 * (g * g)
    assert np.array_equal(wm, pm) and np.array_equal(wv, pv)
    assert np.array_equal(wp, p * factor - (lr2 / c1) * (pm / (np.sqrt(pv) / c2 + eps)))

    # the tick: running products in float64, not pow; within one float32 ulp of the closed form
    assert b1t == (np.float64(b1) * np.float64(b1)) * np.float64(b1) and b2t == (np.float64(b2) * np.float64(b2)) * np.float64(b2)
    assert c1 == f(1.0 - b1t) and c2 == f(np.sqrt(1.0 - b2t))
    assert abs(float(c1) - float(f(1 - float(b1) ** 3))) <= float(np.spacing(c1))
    assert abs(float(c2) - float(f(np.sqrt(1 - float(b2) ** 3)))) <= float(np.spacing(c2))
    # zeros stay zeros (the padding elements of the padded layout)
    z = np.zeros(4, dtype=f)
    for dec in (False, True):
        zp, zm, zv = adam_update(z, z, z, z, lr, c1, c2, b1, b2, eps, wd, dec)
        assert not zp.any() and not zm.any() and not zv.any()


def test_null_net_is_refused_without_a_gpu(libx):
    flat = (C.c_float * 4)()
    b1, b2, eps, wd, dec, sel, step = C.c_float(), C.c_float(), C.c_float(), C.c_float(), C.c_int(), C.c_int(), C.c_int64()
    assert libx.rcn_hipx_set_adam(None, 0.9, 0.999, 1e-8, 0.0, 0) == -1
    assert libx.rcn_hipx_get_adam(None, C.byref(b1), C.byref(b2), C.byref(eps), C.byref(wd), C.byref(dec), C.byref(sel)) == -1
    assert libx.rcn_hipx_get_adam_state(None, flat, flat, C.byref(step)) == -1
    assert libx.rcn_hipx_set_adam_state(None, flat, flat, 0) == -1
    assert libx.rcn_hipx_reset_adam(None) == -1


def test_header_declares_adam_and_the_binding_table_has_it(libx):
    from mercer_research_amd import convnet
    text = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    declared = set(re.findall(r"\b(rcn_hipx_[a-z0-9_]+)\s*\(", text))
    raw = C.CDLL(convnet.LIBX_PATH)
    for name in NEW:
        assert name in declared and name in convnet.SIGNATURES and hasattr(raw, name), name
