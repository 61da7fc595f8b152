"""Track-X gradient clipping by global norm (include/rcn_hipx.h, rcn_hipx_set_clip) restated in NumPy: the sums in float64 in the library's
order (4096-element blocks, four elements per thread, halving trees), everything else in float32 with one rounding per operation, so that it
reproduces k_grad_sumsq, the coefficient and the clipped gradient bit for bit.  It is torch.nn.utils.clip_grad_norm_(params, max_norm) with
the norm accumulated in double."""
from fractions import Fraction

import numpy as np

BLOCK, THREADS = 4096, 1024


def _tree(s):
    """the halving tree over the last axis (THREADS long): strides 512 .. 1, s[t] += s[t + stride] for t < stride; returns s[..., 0]"""
    st = THREADS // 2
    while st >= 1:
        s[..., :st] = s[..., :st] + s[..., st:2 * st]
        st //= 2
    return s[..., 0].copy()


def _scaled(g, scale):
    g = np.ascontiguousarray(g, dtype=np.float32).ravel()
    with np.errstate(all="ignore"):
        return (np.float32(scale) * g).astype(np.float32)


def grad_sumsq(g, scale=1.0):
    """S, a float64: the sum of squares of fl(scale * g) in the library's order.  g: float32, size % 4 == 0 (the padded flat layout)."""
    x = _scaled(g, scale)
    n = x.size
    assert n % 4 == 0
    nb = (n + BLOCK - 1) // BLOCK
    with np.errstate(all="ignore"):
        pad = np.zeros(nb * BLOCK, dtype=np.float64)
        pad[:n] = x.astype(np.float64)
        q = (pad * pad).reshape(nb, THREADS, 4)
        part = _tree((q[:, :, 0] + q[:, :, 1]) + (q[:, :, 2] + q[:, :, 3])) if nb else np.zeros(0, dtype=np.float64)
        # acc[t] = partial[t] + partial[t + 1024] + ..., sequentially
        acc = np.zeros(THREADS, dtype=np.float64)
        for lo in range(0, nb, THREADS):
            row = part[lo:lo + THREADS]
            acc[:row.size] = acc[:row.size] + row
        return np.float64(_tree(acc))


def grad_norm(g, scale=1.0):
    """norm, a float32: the double square root of S rounded once"""
    with np.errstate(all="ignore"):
        return np.float32(np.sqrt(grad_sumsq(g, scale)))


def clip_coef(norm, max_norm):
    """coef = min(1, max_norm / (norm + 1e-6)) in float32; a NaN stays a NaN (torch.clamp(max=1))"""
    with np.errstate(all="ignore"):
        return np.float32(np.minimum(np.float32(1), np.float32(max_norm) / (np.float32(norm) + np.float32(1e-6))))


def apply_coef(g, coef, scale=1.0):
    """g' = fl(coef * fl(scale * g)), float32, the shape of g"""
    with np.errstate(all="ignore"):
        return (np.float32(coef) * _scaled(g, scale)).astype(np.float32).reshape(np.shape(g))


def clip(g, max_norm, scale=1.0):
    """(g', norm, coef) of one padded flat gradient"""
    norm = grad_norm(g, scale)
    coef = clip_coef(norm, max_norm)
    return apply_coef(g, coef, scale), norm, coef


def plain_update(p, g, lr):
    """The DEFAULT optimiser's update as its kernels have always computed it: p - lr * g rounded ONCE (a fused multiply-add; k_reduce_all,
    k_axpy), where _sgd_ref.sgd_update with momentum = weight_decay = 0 rounds the product and the difference.  float32 in, float32 out.
    The product of two float32 values is exact in float64; the float64 sum rounds once more, which can only matter where it lands exactly
    half way between two float32 values: those elements are redone in exact rational arithmetic."""
    p, g = np.ascontiguousarray(p, dtype=np.float32), np.ascontiguousarray(g, dtype=np.float32)
    with np.errstate(all="ignore"):
        s = p.astype(np.float64) - np.float64(np.float32(lr)) * g.astype(np.float64)
        out = s.astype(np.float32)
    tie = np.isfinite(s) & ((s.view(np.int64) & ((1 << 29) - 1)) == (1 << 28))
    for i in np.flatnonzero(tie):
        exact = Fraction(float(p.flat[i])) - Fraction(float(np.float32(lr))) * Fraction(float(g.flat[i]))
        lo, hi = sorted((np.nextafter(out.flat[i], np.float32(-np.inf)), np.nextafter(out.flat[i], np.float32(np.inf))))
        out.flat[i] = min((out.flat[i], lo, hi), key=lambda c: abs(Fraction(float(c)) - exact))      # (an exact tie keeps the even one)
    return out
