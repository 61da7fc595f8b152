"""The Track-X optimiser (include/rcn_hipx.h, rcn_hipx_set_sgd) restated in NumPy: torch.optim.SGD with dampening 0, every operation in
the array's own precision and in the library's order, so that on float32 arrays it reproduces the GPU update bit for bit."""
import numpy as np


def sgd_update(p, g, v, lr, momentum=0.0, weight_decay=0.0, nesterov=False, grad_scale=1.0):
    """One step on flat arrays of one dtype; returns (new p, new v).  v: the velocity (zeros before the first step)."""
    t = p.dtype.type
    mu, wd, lr, gs = t(momentum), t(weight_decay), t(lr), t(grad_scale)
    d = gs * g
    if wd != 0:
        d = d + wd * p
    if mu != 0:
        v = mu * v + d
        d = d + mu * v if nesterov else v
    p = p - lr * d
    return p, v
