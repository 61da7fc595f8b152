"""The reference of the global-average-pooling tests: tests/_res_ref.py's float64 torch twin with a ("global_avgpool",) layer,
t.mean((2, 3)) = torch.nn.AdaptiveAvgPool2d(1) + flatten(1), after which the dense layer sees [B][C].  tests/_bn_ref.py's shape walk does not
know the kind, so the walk, the flat layouts and the per-tensor comparison built on them are restated here; everything else is the twin's.
Also the exact cases of tests/test_convnet_gap_plan.py / tests/test_gpu_convnet_gap.py: integer nets on which the pool's sums and its
division are exact in fp32.  Not a test file: every assert carries its message."""
import _bn_ref
import numpy as np
from _bn_ref import close  # noqa: F401  (for the test files)
from _res_ref import ResTorchNet, plain, skips

NO_PARAMS = ("pool", "global_avgpool")


def param_shapes(in_shape, layers):
    """[(K, Cout)] of every layer with parameters, in order: _bn_ref's walk, and a global_avgpool layer ends the map (the dense layer
    behind it has K = C)"""
    H, W, C = in_shape
    flat, out = False, []
    for l in plain(layers):
        if l[0] in ("conv", "conv_linear"):
            out.append((9 * C, l[1])); C = l[1]
        elif l[0] == "bn_relu":
            out.append((1, C))
        elif l[0] == "pool":
            H, W = H // 2, W // 2
        elif l[0] == "global_avgpool":
            assert not flat, "global_avgpool behind the dense stage"
            flat = True
        else:
            out.append((C if flat else H * W * C, l[1])); C, flat = l[1], True
    return out


def tensor_slices(in_shape, layers):
    slices, o = [], 0
    for k, c in param_shapes(in_shape, layers):
        slices.append((slice(o, o + k * c), slice(o + k * c, o + k * c + c)))
        o += k * c + c
    return slices


def n_logical(in_shape, layers):
    return tensor_slices(in_shape, layers)[-1][1].stop


def random_params(rng, in_shape, layers):
    """_bn_ref.random_params' draws over this file's shapes"""
    flat = []
    for (k, c), kind in zip(param_shapes(in_shape, layers), [l[0] for l in plain(layers) if l[0] not in NO_PARAMS]):
        if kind == "bn_relu":
            flat += [1.0 + 0.3 * rng.standard_normal(c), 0.2 * rng.standard_normal(c)]
        else:
            flat += [(rng.standard_normal((k, c)) * np.sqrt(2.0 / k)).ravel(), rng.standard_normal(c) * 0.1]
    return np.concatenate(flat).astype(np.float32)


def close_per_tensor(got, ref, in_shape, layers, rtol, tag="", widened=None):
    """_bn_ref.close on every layer's weights (gamma) and biases (beta), each at its own scale; returns the worst |d| / allowance.
    widened: {(layer with parameters, "weights" | "biases"): factor} of tensors whose allowance rtol * scale + 1e-6 is multiplied by a
    factor the caller derives and names; their share is of the widened allowance."""
    got, ref = np.asarray(got, dtype=np.float64).ravel(), np.asarray(ref, dtype=np.float64).ravel()
    slices = tensor_slices(in_shape, layers)
    assert got.size == ref.size == slices[-1][1].stop, (got.size, ref.size, slices[-1][1].stop)
    kinds = [l[0] for l in layers if l[0] not in NO_PARAMS]
    worst = 0.0
    for li, pair in enumerate(slices):
        for part, s in zip(("weights", "biases"), pair):
            factor = (widened or {}).get((li, part), 1.0)
            if factor == 1.0:
                worst = max(worst, close(got[s], ref[s], rtol, f"{tag} layer {li} ({kinds[li]}) {part}"))
                continue
            d, allowance = float(np.abs(got[s] - ref[s]).max()), factor * (rtol * max(1e-3, float(np.abs(ref[s]).max())) + 1e-6)
            print(f"{tag} layer {li} ({kinds[li]}) {part}: max |d| = {d:.3e} allowance x {factor:.3f} = {allowance:.3e} used = {d / allowance:.3f} (unwidened: {d * factor / allowance:.3f})")
            assert d <= allowance, (tag, li, part, d, allowance)
            worst = max(worst, d / allowance)
    return worst


class GapTorchNet(ResTorchNet):
    """ResTorchNet of a description with one ("global_avgpool",) layer.  gate_below = False DROPS the ReLU of the layer below the pool on
    the gradient path only (same values; the gradient passes that ReLU as if it were open): what a backward pass without the pool's gate
    computes -- for the gate test, never a model of the library."""

    def __init__(self, in_shape, layers, flat, momentum=0.1, eps=1e-5, operand="f64", gate_below=True):
        import torch
        self.operand, self.gate_source, self.gate_below = operand, True, gate_below
        self.torch, self.in_shape, self.layers = torch, tuple(in_shape), [tuple(l) for l in plain(layers)]
        self.res_layers, self.skips = [tuple(l) for l in layers], skips(layers)
        flat = np.asarray(flat, dtype=np.float64)
        assert flat.size == n_logical(in_shape, layers), (flat.size, n_logical(in_shape, layers))
        self.mods, self.kinds, self.outs = [], [], []
        C = in_shape[2]
        sl = iter(tensor_slices(in_shape, layers))
        for l in self.layers:
            if l[0] in NO_PARAMS:
                self.mods.append(torch.nn.MaxPool2d(2) if l[0] == "pool" else torch.nn.Sequential(torch.nn.AdaptiveAvgPool2d(1), torch.nn.Flatten(1)))
                self.kinds.append(l[0])
                continue
            ws, bs = next(sl)
            if l[0] in ("conv", "conv_linear"):
                m = torch.nn.Conv2d(C, l[1], 3, padding=1).double()
                w = np.ascontiguousarray(flat[ws].reshape(3, 3, C, l[1]).transpose(3, 2, 0, 1))
                C = l[1]
            elif l[0] == "bn_relu":
                m = torch.nn.BatchNorm2d(C, eps=eps, momentum=momentum).double()
                w = flat[ws].copy()
            else:
                k = flat[ws].size // l[1]
                m = torch.nn.Linear(k, l[1]).double()
                w = np.ascontiguousarray(flat[ws].reshape(k, l[1]).T)
            with torch.no_grad():
                m.weight.copy_(torch.from_numpy(w))
                m.bias.copy_(torch.from_numpy(flat[bs].copy()))
            self.mods.append(m); self.kinds.append(l[0])
        self.gap_at = self.kinds.index("global_avgpool")
        assert self.kinds.count("global_avgpool") == 1 and self.gap_at >= 1, self.kinds

    def forward(self, x, train):
        torch = self.torch
        self._mode(train)
        t = torch.from_numpy(np.ascontiguousarray(np.asarray(x, dtype=np.float64).transpose(0, 3, 1, 2)))
        self.outs = []
        for i, (kind, m) in enumerate(zip(self.kinds, self.mods)):
            if kind in ("dense", "dense_relu") and t.dim() == 4:
                t = t.permute(0, 2, 3, 1).reshape(t.shape[0], -1)
            if kind == "global_avgpool":
                assert t.dim() == 4, "global_avgpool needs a map"
                assert torch.allclose(t.detach().mean((2, 3)), m(t.detach()), rtol=1e-14, atol=0), "mean((2, 3)) is AdaptiveAvgPool2d(1) + flatten(1)"
                t = t.mean((2, 3))
            else:
                t = self._rounded(m, t) if self.operand == "bf16" and self._is_rounded(kind, m) else m(t)
            if i in self.skips:
                t = t + self.outs[self.skips[i]]
            if kind in ("conv", "bn_relu", "dense_relu"):
                r = torch.relu(t)
                # (the layer below the pool, gate dropped: the ReLU's value with the pre-activation's gradient)
                t = r if self.gate_below or i != self.gap_at - 1 else r.detach() + t - t.detach()
            self.outs.append(t)
        return t

    def _flat(self, of):
        out = []
        for kind, m in zip(self.kinds, self.mods):
            if kind in NO_PARAMS:
                continue
            w, b = of(m.weight).detach().numpy(), of(m.bias).detach().numpy()
            if kind in ("conv", "conv_linear"):
                w = w.transpose(2, 3, 1, 0).reshape(-1, w.shape[0])
            elif kind != "bn_relu":
                w = w.T
            out += [np.ascontiguousarray(w).ravel(), b.ravel()]
        return np.concatenate(out)


# ---- exact nets: (H, W, 3) -> conv C -> global_avgpool -> dense classes, H * W a power of two ------------------------------------------------

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
