"""Track-X gradient accumulation (include/rcn_hipx.h, rcn_hipx_set_accumulate) restated in NumPy: float32, one rounding per operation, in
the library's order, so that it reproduces the accumulator bit for bit.  With c = fl(1.0f / k):
    acc = fl(c * g_0)                   a store
    acc = fl(acc + fl(c * g_j))         j = 1 .. k - 1, in order
It is (loss / k).backward() k times on float32 gradients."""
import numpy as np


def scale_of(k):
    """c, a float32: 1 / k rounded once"""
    return np.float32(1.0) / np.float32(k)


def accumulate(grads, k):
    """acc after the micro-batches of `grads` (float32 arrays of one shape; at most k of them: fewer is a cycle still open)"""
    grads = [np.ascontiguousarray(g, dtype=np.float32) for g in grads]
    assert 1 <= len(grads) <= int(k)
    c = scale_of(k)
    with np.errstate(all="ignore"):
        acc = (c * grads[0]).astype(np.float32)
        for g in grads[1:]:
            acc = (acc + (c * g).astype(np.float32)).astype(np.float32)
    return acc
