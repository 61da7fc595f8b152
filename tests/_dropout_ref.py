"""Track-X dropout (include/rcn_hipx.h, rcn_hipx_set_dropout) restated in NumPy.

The draw, in wrapping uint64 arithmetic on arrays: element idx of site d in the training forward with ordinal t
    z = seed ^ (t * 0xD1342543DE82EF95);   z += ((((uint64)d << 48) + idx) + 1) * 0x9E3779B97F4A7C15
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9;  z = (z ^ (z >> 27)) * 0x94D049BB133111EB;  z ^= z >> 31
    keep = (uint32)(z >> 40) >= thr,        thr = llrint((double)p * 2^24),   s = fl(1.0f / fl(1.0f - p))
the float32 forward a' = keep ? fl(a * s) : +0.0f and backward fl(g * s), one rounding each, and an f64 loss_and_grads: the forward and
backward of oracle/convnet_oracle.py with a' = a * mask * s behind every dense_relu layer."""
import numpy as np

from oracle import convnet_oracle as co

# (4, 8, 3) -> conv 128 -> pool -> 128 -> 32 -> 3 classes at B = 130: site 0 is gated by the input-gradient kernel of the layer above it, site 1
# sits under the fused head, and B is no multiple of 8 or 32
TWO_SITES = ((4, 8, 3), (("conv", 128), ("pool",), ("dense_relu", 128), ("dense_relu", 32), ("dense", 3)), 130)

_M64 = (1 << 64) - 1


def threshold(p):
    """thr: a drop has probability thr / 2^24 (p as the library holds it, a float32)"""
    return int(np.rint(np.float64(np.float32(p)) * 16777216.0))


def scale(p):
    """s, a float32: 1 / (1 - p), each of the two operations rounded once"""
    return np.float32(1.0) / (np.float32(1.0) - np.float32(p))


def keep(p, seed, t, site, count, first=0):
    """bool array: are elements first .. first + count - 1 of `site` kept in the forward with ordinal t?"""
    u = np.uint64
    with np.errstate(over="ignore"):
        stem = np.full(int(count), (int(seed) & _M64) ^ ((int(t) * 0xD1342543DE82EF95) & _M64), dtype=u)
        q = np.arange(int(first), int(first) + int(count), dtype=u) + u((int(site) << 48) & _M64)
        z = stem + (q + u(1)) * u(0x9E3779B97F4A7C15)
        z = (z ^ (z >> u(30))) * u(0xBF58476D1CE4E5B9)
        z = (z ^ (z >> u(27))) * u(0x94D049BB133111EB)
        z = z ^ (z >> u(31))
    return (z >> u(40)).astype(np.uint32) >= np.uint32(threshold(p))


def masks_of(p, seed, t, layers, B):
    """the keep masks [B, units] of every site of `layers` at ordinal t, in site order"""
    units = [l[1] for l in layers if l[0] == "dense_relu"]
    return [keep(p, seed, t, d, B * U).reshape(B, U) for d, U in enumerate(units)]


def forward32(a, kept, p):
    """a' = keep ? fl(a * s) : +0.0f on float32 arrays"""
    a = np.ascontiguousarray(a, dtype=np.float32)
    with np.errstate(all="ignore"):
        return np.where(kept, (a * scale(p)).astype(np.float32), np.float32(0.0)).astype(np.float32)


def backward32(g, p):
    """fl(g * s) on float32 arrays (g: the gradient already gated by a' > 0)"""
    with np.errstate(all="ignore"):
        return (np.ascontiguousarray(g, dtype=np.float32) * scale(p)).astype(np.float32)


def loss_and_grads(x, labels, ws, bs, layers, masks, operand="f64", s=1.0, head32=None):
    """co.loss_and_grads (stored=False) with a' = a * mask * s behind each dense_relu layer; masks: one [B, units] array per site, in site
    order; s: the scale as the device holds it.  (loss, logits, gws, gbs), all f64.  Downstream of a site everything reads a': the next
    layer's forward and weight gradient, and the ReLU gate, a' > 0; the gated gradient that comes back is scaled by s.
    operand: co's rule ("bf16": GEMM operands rounded, except a first layer of one k-block and the fused head).  head32: does the logits
    layer run fp32 arithmetic in bf16 mode?  None: co.head_is_fp32(layers), the rule by shape, which holds while the head is the fused
    one; False for a net whose `head` option is off, where that layer runs on the bf16 GEMM kernels like any other."""
    head32 = co.head_is_fp32(layers) if head32 is None else bool(head32)
    s = float(s)
    a = np.asarray(x, dtype=np.float64)
    cache, pi, site = [], 0, 0
    for li, l in enumerate(layers):
        if l[0] == "conv":
            N, H, W, C = a.shape
            cols = co._im2col(a)
            op = "f64" if cols.shape[1] <= 32 else operand
            y = np.maximum(co._op(cols, op) @ co._op(ws[pi], op) + bs[pi], 0).reshape(N, H, W, -1)
            cache.append(("conv", cols, y, a.shape))
            a = y; pi += 1
        elif l[0] == "pool":
            N, H, W, C = a.shape
            win = a.reshape(N, H // 2, 2, W // 2, 2, C).transpose(0, 1, 3, 2, 4, 5).reshape(N, H // 2, W // 2, 4, C)
            idx = win.argmax(axis=3)
            cache.append(("pool", idx, a.shape))
            a = np.take_along_axis(win, idx[:, :, :, None, :], axis=3)[:, :, :, 0, :]
        else:
            f = a.reshape(a.shape[0], -1)
            op = "f64" if (li == len(layers) - 1 and head32) else operand
            z = co._op(f, op) @ co._op(ws[pi], op) + bs[pi]
            if l[0] == "dense_relu":
                y = np.maximum(z, 0) * np.asarray(masks[site], dtype=np.float64) * s
                site += 1
            else:
                y = z
            cache.append((l[0], f, y, a.shape))
            a = y; pi += 1
    logits = a
    B = logits.shape[0]
    z = logits - logits.max(axis=1, keepdims=True)
    p = np.exp(z); p /= p.sum(axis=1, keepdims=True)
    loss = float(-np.log(p[np.arange(B), labels]).mean())
    d = p.copy(); d[np.arange(B), labels] -= 1.0; d /= B
    gws, gbs = [None] * len(ws), [None] * len(bs)
    pi = len(ws) - 1
    for bi, c in enumerate(reversed(cache)):
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
            gws[pi] = cols.T @ dz if small else co._op(cols, operand).T @ co._op(dz, operand); gbs[pi] = dz.sum(axis=0)
            dcols = (co._op(dz, operand) @ co._op(ws[pi], operand).T).reshape(N, H, W, 9, C)
            dxp = np.zeros((N, H + 2, W + 2, C))
            t = 0
            for kh in range(3):
                for kw in range(3):
                    dxp[:, kh:kh + H, kw:kw + W, :] += dcols[:, :, :, t, :]; t += 1
            d = dxp[:, 1:-1, 1:-1, :]
            pi -= 1
        else:
            kind, f, y, shp = c
            dz = d * (y > 0) * s if kind == "dense_relu" else d      # y = a': positive exactly where the element was kept and a > 0
            op = "f64" if (bi == 0 and head32) else operand
            gws[pi] = co._op(f, op).T @ co._op(dz, op); gbs[pi] = dz.sum(axis=0)
            d = (co._op(dz, op) @ co._op(ws[pi], op).T).reshape(shp)
            pi -= 1
    return loss, logits, gws, gbs
