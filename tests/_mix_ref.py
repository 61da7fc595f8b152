"""Host restatements for the label-smoothing and mixup / CutMix tests (include/rcn_hipx.h: rcn_hipx_set_loss, rcn_hipx_mix_step): the mixed
batch built from tests/_recipe_ref.py's augmented rows with one np.float32 operation per rounding, the dense soft target, and the oracle's
loss and backward walk (oracle/convnet_oracle.py) restated from d = (p - T) / B for a dense target matrix T.  Nothing here calls the library.
tests/test_convnet_mix_plan.py pins soft_loss_and_grads to the oracle bit for bit (one-hot T) and to finite differences (soft T)."""
import numpy as np
from _convnet_util import CIFAR, FUSED_HEAD, ODD_WIDTH, PLAIN_HEAD, POOL_PAIRS  # noqa: F401  (the nets: its importers take them from here too)
from _recipe_ref import augment_ref

from oracle import convnet_oracle as co


def mix_rows(a, rec):
    """a: [B, H, W, C] float32, what the un-mixed gather writes for the batch (row r at position q0 + r).  rec: (blend, weight, y0, y1, x0, x1).
    Row r is mixed with row B - 1 - r: inside the box the partner's value, else a at blend 1, else fl(fl(blend * a) + fl(fl(1 - blend) * b))."""
    blend, _, y0, y1, x0, x1 = rec
    a = np.ascontiguousarray(a, dtype=np.float32)
    b = a[::-1]
    _, H, W, _ = a.shape
    hh, ww = np.arange(H)[:, None], np.arange(W)[None, :]
    inside = ((hh >= y0) & (hh < y1) & (ww >= x0) & (ww < x1))[None, :, :, None]
    bl = np.float32(blend)
    if bl == np.float32(1.0):
        blended = a
    else:
        pa = (bl * a).astype(np.float32)
        pb = ((np.float32(1.0) - bl).astype(np.float32) * b).astype(np.float32)
        blended = (pa + pb).astype(np.float32)
    return np.where(inside, b, blended).astype(np.float32)


def gather_mix_ref(rows, rec, widen, aug=None, q0=0):
    """rows: [B, H, W, C] STORED values (uint8 or float32), already gathered in batch order; aug: None or (pad, hflip, seed, epoch), row r
    drawing with q0 + r; widen: stored -> float32 (the gather's two roundings for uint8)."""
    stored = rows if aug is None else augment_ref(rows, aug[0], aug[1], aug[2], aug[3], q0)
    return mix_rows(widen(stored), rec)


def soft_targets(ya, yb, w, eps, C):
    """T[s][c] = (1 - eps) * (w [c == ya[s]] + (1 - w) [c == yb[s]]) + eps / C, in f64"""
    ya, yb = np.asarray(ya), np.asarray(yb)
    B = ya.shape[0]
    oa, ob = np.zeros((B, C)), np.zeros((B, C))
    oa[np.arange(B), ya] = 1.0
    ob[np.arange(B), yb] = 1.0
    return (1.0 - eps) * (w * oa + (1.0 - w) * ob) + eps / C


def soft_loss_f64(logits, ya, yb, w, eps):
    """the header's loss formula in f64 on given logits: mean over samples of -((1-eps)(w lp_ya + (1-w) lp_yb) + (eps/C) sum_c lp_c)"""
    z = np.asarray(logits, dtype=np.float64)
    B, C = z.shape
    zm = z - z.max(axis=1, keepdims=True)
    lp = zm - np.log(np.exp(zm).sum(axis=1, keepdims=True))
    r = np.arange(B)
    return float(np.mean(-((1.0 - eps) * (w * lp[r, ya] + (1.0 - w) * lp[r, yb]) + (eps / C) * lp.sum(axis=1))))


def soft_loss_and_grads(x, T, ws, bs, layers, operand="f64", stored=False):
    """convnet_oracle.loss_and_grads for a dense target T [B, C]: loss = mean_s -sum_c T[s][c] log p[s][c] (terms with T == 0 are dropped),
    d logits = (p - T) / B, then the oracle's backward walk, statement for statement."""
    cache = []
    logits = co.forward(x, ws, bs, layers, cache, operand, stored)
    B = logits.shape[0]
    z = logits - logits.max(axis=1, keepdims=True)
    p = np.exp(z); p /= p.sum(axis=1, keepdims=True)
    T = np.asarray(T, dtype=np.float64)
    with np.errstate(divide="ignore", invalid="ignore"):
        terms = np.where(T != 0, T * np.log(p), 0.0)
    loss = float((-terms.sum(axis=1)).mean())
    d = (p - T) / B
    gws, gbs = [None] * len(ws), [None] * len(bs)
    pi = len(ws) - 1
    head32 = co.head_is_fp32(layers)
    _op = co._op
    for bi, (l, c) in enumerate(zip(reversed(layers), reversed(cache))):
        if c[0] == "pool":
            _, idx, shp = c
            N, H, W, C = shp
            g = np.zeros((N, H // 2, W // 2, 4, C))
            np.put_along_axis(g, idx[:, :, :, None, :], d[:, :, :, None, :], axis=3)
            d = g.reshape(N, H // 2, W // 2, 2, 2, C).transpose(0, 1, 3, 2, 4, 5).reshape(N, H, W, C)
        elif c[0] == "conv":
            _, cols, y, shp = c
            N, H, W, C = shp
            dz = (d * (y > 0)).reshape(N * H * W, -1)
            small = cols.shape[1] <= 32
            gws[pi] = cols.T @ dz if small else _op(cols, operand).T @ _op(dz, operand); gbs[pi] = dz.sum(axis=0)
            dcols = (_op(dz, operand) @ _op(ws[pi], operand).T).reshape(N, H, W, 9, C)
            dxp = np.zeros((N, H + 2, W + 2, C))
            t = 0
            for kh in range(3):
                for kw in range(3):
                    dxp[:, kh:kh + H, kw:kw + W, :] += dcols[:, :, :, t, :]; t += 1
            d = dxp[:, 1:-1, 1:-1, :]
            pi -= 1
        else:
            kind, f, y, shp = c
            dz = d * (y > 0) if kind == "dense_relu" else d
            op = "f64" if (bi == 0 and head32) else operand
            gws[pi] = _op(f, op).T @ _op(dz, op); gbs[pi] = dz.sum(axis=0)
            d = (_op(dz, op) @ _op(ws[pi], op).T).reshape(shp)
            pi -= 1
        li = len(layers) - 1 - bi
        if stored and c[0] != "pool" and li > 0 and layers[li - 1][0] in ("conv", "pool"):
            d = co.round_bf16(d)
    return loss, logits, gws, gbs
