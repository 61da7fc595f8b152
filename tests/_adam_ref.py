"""Track-X Adam and AdamW (include/rcn_hipx.h, rcn_hipx_set_adam) restated in NumPy: torch.optim.Adam (L2 form) and torch.optim.AdamW, the
tick in float64 as running products, the update with every operation in the array's own precision and in the library's order, so that on
float32 arrays it reproduces the GPU update bit for bit."""
import numpy as np

TICK0 = (0, np.float64(1.0), np.float64(1.0))           # (step, b1t, b2t) before the first update


def adam_tick(state, b1, b2, dtype=np.float32):
    """One tick of state = (step, b1t, b2t): returns (state', c1, c2).  b1, b2 are the float32 betas; the products run in float64 (no
    pow); c1 = 1 - b1t and c2 = sqrt(1 - b2t) are computed in float64 and rounded once to `dtype` (the library: float32)."""
    step, b1t, b2t = state
    b1t = np.float64(b1t) * np.float64(np.float32(b1))
    b2t = np.float64(b2t) * np.float64(np.float32(b2))
    c1 = dtype(np.float64(1.0) - b1t)
    c2 = dtype(np.sqrt(np.float64(1.0) - b2t))
    return (step + 1, b1t, b2t), c1, c2


def adam_ticks(step, b1, b2, dtype=np.float32):
    """the state after `step` ticks from TICK0 with its (c1, c2): what rcn_hipx_set_adam_state rebuilds"""
    state, c1, c2 = TICK0, dtype(0), dtype(0)
    for _ in range(step):
        state, c1, c2 = adam_tick(state, b1, b2, dtype)
    return state, c1, c2


def adam_update(p, g, m, v, lr, c1, c2, b1=0.9, b2=0.999, eps=1e-8, weight_decay=0.0, decoupled=False):
    """One update on flat arrays of one dtype; returns (new p, new m, new v).  c1, c2: this update's bias corrections (adam_tick).  The
    constants are formed in float32 as the library's host does (b1 = (float)beta1, a1 = fl(1.0f - b1), ...) and then taken to the arrays'
    dtype; on float64 arrays a1 = 1 - b1 is formed in float64 (torch's 1 - beta1)."""
    t = p.dtype.type
    f = np.float32
    b1, b2 = f(b1), f(b2)
    a1, a2 = (f(1) - b1, f(1) - b2) if t is np.float32 else (t(1) - t(b1), t(1) - t(b2))
    b2, eps, wd, lr, c1, c2 = t(b2), t(eps), t(weight_decay), t(lr), t(c1), t(c2)
    with np.errstate(all="ignore"):
        x = g
        if wd != 0:
            if decoupled:
                p = p * (t(1) - lr * wd)
            else:
                x = x + wd * p
        m = m + a1 * (x - m)
        v = b2 * v + a2 * (x * x)
        d = np.sqrt(v) / c2 + eps
        p = p - (lr / c1) * (m / d)
    return p, m, v
