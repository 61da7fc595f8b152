"""NumPy restatement of what rcn_hipx_evaluate_metrics_dev computes from logits (include/rcn_hipx.h), for tests/test_convnet_eval_metrics.py
(CPU) and tests/test_gpu_convnet_eval_metrics.py (GPU).  Not a test file and not a conftest: every assert carries its message."""
import numpy as np


def rank(logits, y):
    """[n] int32: how many classes BEAT row i's label y[i] -- class c beats y when z[c] > z[y], or z[c] == z[y] and c < y; -1 for a label
    outside [0, classes)"""
    z, y = np.asarray(logits), np.asarray(y).astype(np.int64)
    n, C = z.shape
    assert y.shape == (n,), (y.shape, n)
    ok = (y >= 0) & (y < C)
    ys = np.where(ok, y, 0)
    zy = z[np.arange(n), ys][:, None]
    c = np.arange(C)[None, :]
    beats = (z > zy) | ((z == zy) & (c < ys[:, None]))
    return np.where(ok, beats.sum(axis=1), -1).astype(np.int32)


def pred(logits):
    """the first maximum of every row"""
    return np.asarray(logits).argmax(axis=1).astype(np.int32)


def topk_counts(ranks, ks):
    """[len(ks)] int64: rows with 0 <= rank < k"""
    r = np.asarray(ranks)
    return np.array([int(((r >= 0) & (r < k)).sum()) for k in ks], dtype=np.int64)


def confusion(y, predicted, classes):
    """[classes, classes] int64, row = label, column = prediction; a label outside [0, classes) is in no cell"""
    y, p = np.asarray(y).astype(np.int64), np.asarray(predicted).astype(np.int64)
    ok = (y >= 0) & (y < classes)
    m = np.zeros((classes, classes), dtype=np.int64)
    np.add.at(m, (y[ok], p[ok]), 1)
    return m


def loss_sum_from_rows(loss_each, max_batch):
    """*loss_sum (float64) rebuilt from the device's per-row floats in the documented order.  Per chunk of max_batch rows: blocks of 8 rows,
    each summed in row order in float32; "thread t" adds blocks t, t + 256, ... in float64; the 256 sums are added in order; the chunks'
    totals are added in chunk order."""
    rows = np.asarray(loss_each)
    assert rows.dtype == np.float32 and rows.ndim == 1, (rows.dtype, rows.shape)
    total = np.float64(0.0)
    for off in range(0, rows.size, max_batch):
        chunk = rows[off:off + max_batch]
        blocks = []
        for b in range(0, chunk.size, 8):
            t = np.float32(0.0)
            for v in chunk[b:b + 8]:
                t = np.float32(t + v)
            blocks.append(t)
        threads = []
        for t in range(256):
            acc = np.float64(0.0)
            for v in blocks[t::256]:
                acc = acc + np.float64(v)
            threads.append(acc)
        tot = np.float64(0.0)
        for v in threads:
            tot = tot + v
        total = total + tot
    return np.float64(total)


def step_loss_from_rows(loss_each):
    """A training step's loss (float32) rebuilt from the per-row floats of its batch in the loss kernel's order: blocks of 8 rows, each summed
    in row order; "thread t" adds blocks t, t + 256, ...; the 256 sums are added in order; the total times fl(1 / B).  All in float32."""
    rows = np.asarray(loss_each)
    assert rows.dtype == np.float32 and rows.ndim == 1, (rows.dtype, rows.shape)
    blocks = []
    for b in range(0, rows.size, 8):
        t = np.float32(0.0)
        for v in rows[b:b + 8]:
            t = np.float32(t + v)
        blocks.append(t)
    tot = np.float32(0.0)
    for t in range(256):
        acc = np.float32(0.0)
        for v in blocks[t::256]:
            acc = np.float32(acc + v)
        tot = np.float32(tot + acc)
    return np.float32(tot * (np.float32(1.0) / np.float32(rows.size)))


def cross_entropy(logits, y):
    """[n] float64 soft-max cross-entropy of every row with a label inside [0, classes); 0 for the others"""
    z = np.asarray(logits, dtype=np.float64)
    y = np.asarray(y).astype(np.int64)
    ok = (y >= 0) & (y < z.shape[1])
    z = z - z.max(axis=1, keepdims=True)
    logp = z - np.log(np.exp(z).sum(axis=1, keepdims=True))
    return np.where(ok, -logp[np.arange(len(y)), np.where(ok, y, 0)], 0.0)
