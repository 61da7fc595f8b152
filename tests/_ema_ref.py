"""The Track-X average of the parameters (include/rcn_hipx.h, rcn_hipx_set_ema) restated in NumPy: e <- e + a * (p - e) with
a = 1 - decay computed once, every operation in the array's own precision and in the library's order, so that on float32 arrays it
reproduces the GPU update bit for bit.  It is torch.lerp(e, p, 1 - decay) in its weight < 0.5 form."""
import numpy as np


def ema_update(e, p, decay):
    """One update on flat arrays of one dtype; returns the new e.  On float32 arrays a = np.float32(1) - np.float32(decay)."""
    t = e.dtype.type
    a = t(1) - t(decay)
    d = p - e
    return e + a * d
