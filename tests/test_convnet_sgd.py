"""CPU checks of the Track-X optimiser (include/rcn_hipx.h, rcn_hipx_set_sgd): the NumPy restatement the GPU tests compare with is
torch.optim.SGD's update, and the new entry points exist, are bound and refuse a null net without a GPU."""
import ctypes as C
import re

import numpy as np
import pytest
from _sgd_ref import sgd_update
from _convnet_util import HEADER, libx  # noqa: F401  (libx: a fixture)

NEW = ["rcn_hipx_set_sgd", "rcn_hipx_get_sgd", "rcn_hipx_get_velocity", "rcn_hipx_set_velocity", "rcn_hipx_reset_velocity", "rcn_hipx_apply_sgd_dev"]


@pytest.mark.parametrize("momentum,weight_decay,nesterov", [(0.9, 5e-4, False), (0.9, 5e-4, True), (0.0, 5e-4, False)])
def test_restatement_is_torch_sgd(momentum, weight_decay, nesterov):
    import torch
    rng = np.random.default_rng(3)
    p0 = rng.standard_normal(257)
    lr = 0.05
    tp = torch.tensor(p0, dtype=torch.float64, requires_grad=True)
    opt = torch.optim.SGD([tp], lr=lr, momentum=momentum, weight_decay=weight_decay, nesterov=nesterov, dampening=0.0)
    p, v = p0.copy(), np.zeros_like(p0)
    for _ in range(6):
        g = rng.standard_normal(p0.size)
        tp.grad = torch.tensor(g, dtype=torch.float64)
        opt.step()
        p, v = sgd_update(p, g, v, lr, momentum, weight_decay, nesterov)
        ref = tp.detach().numpy()
        assert np.abs(p - ref).max() <= 1e-12 * np.abs(ref).max()
        if momentum:
            buf = opt.state[tp]["momentum_buffer"].numpy()
            assert np.abs(v - buf).max() <= 1e-12 * np.abs(buf).max()


def test_restatement_rounds_every_operation_in_float32():
    p = np.array([1.0, -2.5, 3e-3], dtype=np.float32)
    g = np.array([0.1, 0.2, -0.3], dtype=np.float32)
    v = np.array([0.01, 0.0, -0.02], dtype=np.float32)
    np_, nv = sgd_update(p, g, v, 0.1, 0.9, 5e-4, True, 0.5)
    assert np_.dtype == np.float32 and nv.dtype == np.float32
    f = np.float32
    d = f(0.5) * g
    d = d + f(5e-4) * p
    vv = f(0.9) * v + d
    d = d + f(0.9) * vv
    assert np.array_equal(nv, vv) and np.array_equal(np_, p - f(0.1) * d)


def test_null_net_is_refused_without_a_gpu(libx):
    flat = (C.c_float * 4)()
    mu, wd, nest = C.c_float(), C.c_float(), C.c_int()
    assert libx.rcn_hipx_set_sgd(None, 0.9, 5e-4, 1) == -1
    assert libx.rcn_hipx_get_sgd(None, C.byref(mu), C.byref(wd), C.byref(nest)) == -1
    assert libx.rcn_hipx_apply_sgd_dev(None, C.c_void_p(16), 1.0, 0.1) == -1
    assert libx.rcn_hipx_get_velocity(None, flat) == -1
    assert libx.rcn_hipx_set_velocity(None, flat) == -1
    assert libx.rcn_hipx_reset_velocity(None) == -1


def test_header_declares_the_optimiser_and_the_binding_table_has_it(libx):
    from mercer_research_amd import convnet
    text = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    declared = set(re.findall(r"\b(rcn_hipx_[a-z0-9_]+)\s*\(", text))
    raw = C.CDLL(convnet.LIBX_PATH)
    for name in NEW:
        assert name in declared and name in convnet.SIGNATURES and hasattr(raw, name), name

