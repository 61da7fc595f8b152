"""The exact cases of tests/test_convnet_gap_plan.py and tests/test_gpu_convnet_gap.py: integer nets (H, W, 3) -> conv C -> global_avgpool ->
dense classes, H * W a power of two, on which the pool's sums and its division are exact in fp32.  Data, not a twin.  Not a test file."""
import numpy as np


def im2col(x):
    """[N * H * W][9 * Cin] patches of an NHWC batch (3x3, pad 1), column k = (ky * 3 + kx) * Cin + cin: the library's weight layout"""
    N, H, W, C = x.shape
    p = np.zeros((N, H + 2, W + 2, C), dtype=x.dtype)
    p[:, 1:-1, 1:-1] = x
    return np.stack([p[:, ky:ky + H, kx:kx + W] for ky in range(3) for kx in range(3)], axis=3).reshape(N * H * W, 9 * C)


def exact_forward(x, w0, b0, w1, b1):
    """(map [N][HW][C], mean [N][C], logits) in float64 of conv (ReLU) -> global_avgpool -> dense"""
    N, H, W, _ = x.shape
    a = np.maximum(im2col(np.asarray(x, dtype=np.float64)) @ w0 + b0, 0.0).reshape(N, H * W, -1)
    m = a.sum(1) / (H * W)
    return a, m, m @ w1 + b1


def exact_logit_case(in_shape, C, classes, B, seed=0):
    """Integer inputs in [-2, 2], conv weights in {-1, 0, 1} (about six per column), conv biases 13 .. 16: every map value is a POSITIVE
    integer (at most 12 + 16).  Dense weights in {-1, 0, 1} / 4, biases in {-2, -1, 0} / 4.  (x, y, w0, b0, w1, b1, flat)"""
    rng = np.random.default_rng(seed)
    K = 9 * in_shape[2]
    x = rng.integers(-2, 3, (B,) + tuple(in_shape)).astype(np.float32)
    y = rng.integers(0, classes, B).astype(np.int32)
    w0 = np.where(rng.random((K, C)) < 6 / K, rng.choice([-1.0, 1.0], (K, C)), 0.0)
    b0 = rng.integers(13, 17, C).astype(np.float64)
    w1 = np.where(rng.random((C, classes)) < 6 / C, rng.choice([-1.0, 1.0], (C, classes)), 0.0) / 4
    b1 = rng.integers(-2, 1, classes) / 4
    flat = np.concatenate([w0.ravel(), b0, w1.ravel(), b1]).astype(np.float32)
    return x, y, w0, b0, w1, b1, flat


def exact_gate_case(in_shape, C, classes, pixel, seed=0):
    """ONE sample that is zero but for a 1 at `pixel` = (py, px) of input channel 0, conv weights in [-2, 2], conv biases in {-1, 0, 1, 2}:
    the map is relu(b) away from the pixel and relu(b + w) around it, so gates are open and shut within a channel.  Every feature feeds ONE
    class with weight +-1 / 2 (dense row c has one non-zero), so the pool's gradient is g[c] = w1[c][j(c)] * dlogits[j(c)] EXACTLY, and with
    one sample the dense layer's bias gradient IS dlogits.  The first convolution's weight gradient at (tap, channel 0) then has ONE non-zero
    term: the pool's input gradient at the row that tap reaches from the pixel.  (x, y, w0, b0, w1, b1, flat)"""
    rng = np.random.default_rng(seed)
    K = 9 * in_shape[2]
    x = np.zeros((1,) + tuple(in_shape), dtype=np.float32)
    x[0, pixel[0], pixel[1], 0] = 1.0
    y = rng.integers(0, classes, 1).astype(np.int32)
    w0 = rng.integers(-2, 3, (K, C)).astype(np.float64)
    b0 = rng.integers(-1, 3, C).astype(np.float64)
    w1 = np.zeros((C, classes))
    w1[np.arange(C), rng.integers(0, classes, C)] = rng.choice([-0.5, 0.5], C)
    b1 = rng.integers(-2, 1, classes) / 4
    flat = np.concatenate([w0.ravel(), b0, w1.ravel(), b1]).astype(np.float32)
    return x, y, w0, b0, w1, b1, flat


def rows_seen(in_shape, pixel):
    """{tap index ky * 3 + kx: output row oy * W + ox} of the rows whose patch holds `pixel`"""
    H, W, _ = in_shape
    out = {}
    for ky in range(3):
        for kx in range(3):
            oy, ox = pixel[0] - ky + 1, pixel[1] - kx + 1
            if 0 <= oy < H and 0 <= ox < W:
                out[ky * 3 + kx] = oy * W + ox
    return out
