"""CPU checks of the Track-X average of the parameters (include/rcn_hipx.h, rcn_hipx_set_ema): the NumPy restatement the GPU tests compare
with is torch.optim.swa_utils.AveragedModel's EMA, it rounds every operation in float32, and the new entry points exist, are bound and
refuse a null net without a GPU."""
import ctypes as C
import re

import numpy as np
import pytest
from _ema_ref import ema_update
from _convnet_util import HEADER, libx  # noqa: F401  (libx: a fixture)

NEW = ["rcn_hipx_set_ema", "rcn_hipx_get_ema", "rcn_hipx_get_ema_params", "rcn_hipx_set_ema_params", "rcn_hipx_reset_ema", "rcn_hipx_evaluate_ex_dev"]


@pytest.mark.parametrize("decay", [0.5, 0.9, 0.999, 0.9999])
def test_restatement_is_torch_averaged_model_ema(decay):
    """float64, six updates, 1e-12 relative.  update_parameters is called once before the first change of the parameters: AveragedModel's
    first call copies them, which is the library's copy at the moment the average is switched on."""
    import torch
    from torch.optim.swa_utils import AveragedModel, get_ema_multi_avg_fn
    rng = np.random.default_rng(5)
    model = torch.nn.Linear(16, 16, bias=True).double()
    avg = AveragedModel(model, multi_avg_fn=get_ema_multi_avg_fn(decay))

    def flat(m):
        return np.concatenate([q.detach().numpy().ravel() for q in m.parameters()])

    avg.update_parameters(model)
    e = flat(model).copy()
    assert np.array_equal(flat(avg.module), e)
    for _ in range(6):
        with torch.no_grad():
            for q in model.parameters():
                q.add_(torch.tensor(rng.standard_normal(tuple(q.shape)) * 0.1))
        avg.update_parameters(model)
        e = ema_update(e, flat(model), decay)
        ref = flat(avg.module)
        assert e.dtype == np.float64
        assert np.abs(e - ref).max() <= 1e-12 * np.abs(ref).max(), float(np.abs(e - ref).max())
    assert not np.array_equal(e, flat(model))


def test_restatement_rounds_every_operation_in_float32():
    e = np.array([1.0, -2.5, 3e-3, 0.0], dtype=np.float32)
    p = np.array([1.1, -2.25, -7e-3, 0.0], dtype=np.float32)
    got = ema_update(e, p, 0.999)
    assert got.dtype == np.float32
    f = np.float32
    a = f(1) - f(0.999)
    assert a != f(1 - 0.999)                             # fl(1 - fl(decay)) is not the rounded double difference: the order matters
    d = p - e
    assert d.dtype == np.float32
    want = e + a * d
    assert np.array_equal(got, want)
    # ... and element by element in scalar float32 arithmetic
    for k in range(e.size):
        assert got[k] == f(e[k] + f(a * f(p[k] - e[k])))
    assert got[3] == 0.0                                 # a padding element stays 0
    # one rounding per operation differs from the same line in double, rounded at the end, somewhere on a longer vector
    rng = np.random.default_rng(0)
    e2, p2 = rng.standard_normal(4096).astype(np.float32), rng.standard_normal(4096).astype(np.float32)
    dbl = (e2.astype(np.float64) + (1.0 - 0.999) * (p2.astype(np.float64) - e2.astype(np.float64))).astype(np.float32)
    assert not np.array_equal(ema_update(e2, p2, 0.999), dbl)


def test_null_net_is_refused_without_a_gpu(libx):
    flat = (C.c_float * 4)(1.0, 2.0, 3.0, 4.0)
    d = C.c_float(9.0)
    assert libx.rcn_hipx_set_ema(None, 0.5) == -1
    assert libx.rcn_hipx_get_ema(None, C.byref(d)) == -1 and d.value == 9.0
    assert libx.rcn_hipx_get_ema_params(None, flat) == -1 and list(flat) == [1.0, 2.0, 3.0, 4.0]
    assert libx.rcn_hipx_set_ema_params(None, flat) == -1
    assert libx.rcn_hipx_reset_ema(None) == -1
    for weights in (0, 1, 2):
        assert libx.rcn_hipx_evaluate_ex_dev(None, C.c_void_p(16), 0, 1.0, 0.0, None, 1, weights, None, None, C.c_void_p(16)) == -1


def test_header_declares_the_average_and_the_binding_table_has_it(libx):
    from mercer_research_amd import convnet
    raw_text = open(HEADER).read()
    text = re.sub(r"/\*.*?\*/", "", raw_text, flags=re.S)
    declared = set(re.findall(r"\b(rcn_hipx_[a-z0-9_]+)\s*\(", text))
    raw = C.CDLL(convnet.LIBX_PATH)
    for name in NEW:
        assert name in declared and name in convnet.SIGNATURES and hasattr(raw, name), name
    assert re.search(r"RCN_HIPX_WEIGHTS_LIVE\s*=\s*0\b", text) and re.search(r"RCN_HIPX_WEIGHTS_EMA\s*=\s*1\b", text)
    assert convnet.WEIGHTS == {"live": 0, "ema": 1}
    # evaluate_ex is evaluate's argument list with `weights` after the row count
    ev, ex = convnet.SIGNATURES["rcn_hipx_evaluate_dev"], convnet.SIGNATURES["rcn_hipx_evaluate_ex_dev"]
    assert ex[0] is ev[0] and ex[1] == ev[1][:7] + [C.c_int] + ev[1][7:]
