"""The reference of the batch-normalisation, residual, global-average-pooling and deep-net tests: PyTorch on the CPU in float64, the "twin".
`TorchNet` builds the torch.nn modules of a Track X description from (in_shape, layers, flat logical parameters) -- NHWC <-> NCHW,
W[K][Cout] <-> weight[Cout][Cin][3][3], the mapping tests/test_convnet_exact_nets.py::_torch_net uses -- and hands back logits, loss,
gradients, parameters and running statistics in the library's own flat layouts.  ("conv_linear", n), ("bn_relu",) is Conv2d ->
BatchNorm2d -> ReLU; ("bn_add_relu", d) is y = relu(BatchNorm2d(z) + s), s the output of the layer d places in front (torchvision's
BasicBlock with an identity shortcut); ("global_avgpool",) is t.mean((2, 3)) = AdaptiveAvgPool2d(1) + Flatten(1), after which the dense
layer sees [B][C].  A bn_add_relu layer owns what a bn_relu layer owns -- one K = 1 block [gamma | beta] and running statistics -- so the
flat layouts are those of `plain(layers)`.  Not a test file: every assert carries its message."""
import numpy as np
from _convnet_util import close

NO_PARAMS = ("pool", "global_avgpool")


def plain(layers):
    """the description with every ("bn_add_relu", d) written ("bn_relu",): the same parameters, statistics and flat layouts, no skip"""
    return tuple(("bn_relu",) if l[0] == "bn_add_relu" else tuple(l) for l in layers)


def skips(layers):
    """{index of a bn_add_relu layer: index of its source}"""
    return {i: i - l[1] for i, l in enumerate(layers) if l[0] == "bn_add_relu"}


def kinds_with_params(layers):
    """the kind of every layer with parameters, in order, a bn_add_relu layer as "bn_relu" """
    return [l[0] for l in plain(layers) if l[0] not in NO_PARAMS]


def param_shapes(in_shape, layers):
    """[(K, Cout)] of every layer with parameters, in order; a bn_relu or bn_add_relu layer's block is K = 1: [gamma | beta]; a
    global_avgpool layer ends the map (the dense layer behind it has K = C)"""
    H, W, C = in_shape
    flat, out = False, []
    for l in layers:
        if l[0] in ("conv", "conv_linear"):
            out.append((9 * C, l[1])); C = l[1]
        elif l[0] in ("bn_relu", "bn_add_relu"):
            out.append((1, C))
        elif l[0] == "pool":
            H, W = H // 2, W // 2
        elif l[0] == "global_avgpool":
            assert not flat, "global_avgpool behind the dense stage"
            flat = True
        else:
            assert l[0] in ("dense", "dense_relu"), f"unknown layer kind {l[0]!r}"
            out.append((C if flat else H * W * C, l[1])); C, flat = l[1], True
    return out


def tensor_slices(in_shape, layers):
    """every such layer's (weights, biases) as slices of the logical flat layout"""
    slices, o = [], 0
    for k, c in param_shapes(in_shape, layers):
        slices.append((slice(o, o + k * c), slice(o + k * c, o + k * c + c)))
        o += k * c + c
    return slices


def n_logical(in_shape, layers):
    return tensor_slices(in_shape, layers)[-1][1].stop


def random_params(rng, in_shape, layers):
    """He-scaled weights, biases of 0.1 sigma, gamma around 1 and beta around 0 (neither at its default: a swapped or dropped one shows),
    as the float32 flat vector the device holds"""
    flat = []
    for (k, c), kind in zip(param_shapes(in_shape, layers), kinds_with_params(layers)):
        if kind == "bn_relu":
            flat += [1.0 + 0.3 * rng.standard_normal(c), 0.2 * rng.standard_normal(c)]
        else:
            flat += [(rng.standard_normal((k, c)) * np.sqrt(2.0 / k)).ravel(), rng.standard_normal(c) * 0.1]
    return np.concatenate(flat).astype(np.float32)


def _bf16(t):
    """round to nearest even to bfloat16, kept as float64"""
    return t.float().bfloat16().double()


def _rounded_op(torch):
    """conv2d / linear in float64 on operands rounded to bfloat16, forward and backward, as "bf16" precision rounds them on their way into
    the MFMA: the forward rounds x and W, the input gradient dZ and W, the weight gradient x and dZ; the bias gradient sums dZ as it is."""
    class Rounded(torch.autograd.Function):
        @staticmethod
        def forward(ctx, x, w, b):
            xr, wr = _bf16(x), _bf16(w)
            ctx.save_for_backward(xr, wr)
            return torch.nn.functional.conv2d(xr, wr, b, padding=1) if x.dim() == 4 else xr @ wr.T + b

        @staticmethod
        def backward(ctx, g):
            xr, wr = ctx.saved_tensors
            gr = _bf16(g)
            if xr.dim() == 4:
                return (torch.nn.grad.conv2d_input(xr.shape, wr, gr, padding=1), torch.nn.grad.conv2d_weight(xr, wr.shape, gr, padding=1), g.sum((0, 2, 3)))
            return gr @ wr, gr.T @ xr, g.sum(0)
    return Rounded.apply


class TorchNet:
    """The float64 torch.nn twin of a description.  forward(x, train), loss_and_grads(x, y), sgd_step(x, y, lr) and the flat views.
    self.layers is plain(layers) and self.kinds its kinds (a bn_add_relu layer is "bn_relu" there); self.res_layers is the description as
    given, self.skips its {bn_add_relu layer: source} and self.gap_at the index of its global_avgpool layer or None.
    operand = "bf16": the convolutions and dense layers that "bf16" precision runs on bf16 operands round theirs the same way (all but a
    first layer of 9 * Cin <= 32 and a logits layer of <= 32 classes on a ReLU dense layer of <= 256 units: fp32 by shape); batch
    normalisation, pools and the loss stay float64.
    Two options DROP a ReLU on the gradient path only (same values; the gradient passes that ReLU as if it were open) -- for the gate
    tests, never a model of the library.  gate_source = False: the ReLU of every skip source, on the skip path: what a backward pass
    without the source gate computes the gradient of.  gate_below = False: the ReLU of the layer below the pool: what a backward pass
    without the pool's gate computes."""

    def __init__(self, in_shape, layers, flat, momentum=0.1, eps=1e-5, operand="f64", gate_source=True, gate_below=True):
        import torch
        self.operand, self.gate_source, self.gate_below = operand, gate_source, gate_below
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
        for i, s in self.skips.items():
            assert 0 <= s < i - 1 and self.kinds[i - 1] == "conv_linear", (i, s, self.kinds)
        self.gap_at = self.kinds.index("global_avgpool") if "global_avgpool" in self.kinds else None
        assert self.gap_at is None or (self.kinds.count("global_avgpool") == 1 and self.gap_at >= 1), self.kinds

    def _mode(self, train):
        for m in self.mods:
            m.train(train)

    def forward(self, x, train):
        """logits (a float64 tensor in the graph) of an NHWC batch; train: batch statistics, and the running statistics advance.  Remembers
        every layer's output (self.outs, tensors in the graph) and adds the source's in front of a bn_add_relu layer's ReLU."""
        torch = self.torch
        self._mode(train)
        t = torch.from_numpy(np.ascontiguousarray(np.asarray(x, dtype=np.float64).transpose(0, 3, 1, 2)))
        self.outs, pre = [], []
        for i, (kind, m) in enumerate(zip(self.kinds, self.mods)):
            if kind in ("dense", "dense_relu") and t.dim() == 4:
                t = t.permute(0, 2, 3, 1).reshape(t.shape[0], -1)          # NHWC flatten
            if kind == "global_avgpool":
                assert t.dim() == 4, "global_avgpool needs a map"
                assert torch.allclose(t.detach().mean((2, 3)), m(t.detach()), rtol=1e-14, atol=0), "mean((2, 3)) is AdaptiveAvgPool2d(1) + flatten(1)"
                t = t.mean((2, 3))
            else:
                t = self._rounded(m, t) if self.operand == "bf16" and self._is_rounded(kind, m) else m(t)
            if i in self.skips:
                s = self.skips[i]
                # (gate dropped: the same VALUE as the gated sum, but the gradient of the skip path passes the source's ReLU as if it were open)
                t = t + (self.outs[s] if self.gate_source else self.outs[s].detach() + pre[s] - pre[s].detach())
            pre.append(t)
            if kind in ("conv", "bn_relu", "dense_relu"):
                r = torch.relu(t)
                # (the layer below the pool, gate dropped: the ReLU's value with the pre-activation's gradient)
                t = r if self.gate_below or self.gap_at is None or i != self.gap_at - 1 else r.detach() + t - t.detach()
            self.outs.append(t)
        return t

    def _is_rounded(self, kind, m):
        if kind in ("conv", "conv_linear"):
            return 9 * m.in_channels > 32
        if kind == "dense_relu":
            return True
        if kind != "dense":
            return False
        i = self.mods.index(m)
        fused_head = i > 0 and self.kinds[i - 1] == "dense_relu" and m.out_features <= 32 and m.in_features <= 256 and m.in_features % 32 == 0
        return not fused_head

    def _rounded(self, m, t):
        return _rounded_op(self.torch)(t, m.weight, m.bias)

    def logits(self, x, train=False):
        with self.torch.no_grad():
            return self.forward(x, train).numpy()

    def loss_and_grads(self, x, y, label_smoothing=0.0):
        """(loss, logits, flat gradient) of ONE training forward + backward (the running statistics advance once)"""
        torch = self.torch
        for m in self.mods:
            m.zero_grad()
        z = self.forward(x, True)
        loss = torch.nn.functional.cross_entropy(z, torch.from_numpy(np.asarray(y, dtype=np.int64)), label_smoothing=label_smoothing)
        loss.backward()
        return float(loss.detach()), z.detach().numpy(), self._flat(lambda p: p.grad)

    def parameters(self):
        return [p for m in self.mods for p in m.parameters()]

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

    def params(self):
        return self._flat(lambda p: p)

    def bn_stats(self):
        """all bn_relu layers back to back, mean[C] then var[C] per layer: ConvNet.get_bn_stats's layout"""
        out = [a for kind, m in zip(self.kinds, self.mods) if kind == "bn_relu" for a in (m.running_mean.numpy(), m.running_var.numpy())]
        return np.concatenate(out) if out else np.zeros(0)

    def set_bn_stats(self, stats):
        stats, at = np.asarray(stats, dtype=np.float64), 0
        with self.torch.no_grad():
            for kind, m in zip(self.kinds, self.mods):
                if kind == "bn_relu":
                    c = m.num_features
                    m.running_mean.copy_(self.torch.from_numpy(stats[at:at + c].copy()))
                    m.running_var.copy_(self.torch.from_numpy(stats[at + c:at + 2 * c].copy()))
                    at += 2 * c
        assert at == stats.size, (at, stats.size)

    def sgd_step(self, x, y, lr):
        """one plain SGD step; returns the loss before it"""
        loss, _, _ = self.loss_and_grads(x, y)
        with self.torch.no_grad():
            for p in self.parameters():
                p -= lr * p.grad
        return loss


def close_per_tensor(got, ref, in_shape, layers, rtol, tag="", bias_at_weight_scale=(), widened=None):
    """`close` on every layer's weights (gamma) and biases (beta), each at its own scale, rtol * max(1e-3, max |ref|) + 1e-6; returns the
    worst |d| / allowance.  The caller derives and names either exception.
    bias_at_weight_scale: layers (counted among those with parameters) whose bias gradient is held at the scale of the same layer's WEIGHT
    gradient instead.
    widened: {(layer with parameters, "weights" | "biases"): factor} of tensors whose allowance is multiplied by a factor; their share is
    of the widened allowance."""
    got, ref = np.asarray(got, dtype=np.float64).ravel(), np.asarray(ref, dtype=np.float64).ravel()
    slices = tensor_slices(in_shape, layers)
    assert got.size == ref.size == slices[-1][1].stop, (got.size, ref.size, slices[-1][1].stop)
    kinds = [l[0] for l in layers if l[0] not in NO_PARAMS]
    worst = 0.0
    for li, (ws, bs) in enumerate(slices):
        for part, s in (("weights", ws), ("biases", bs)):
            name = f"{tag} layer {li} ({kinds[li]}) {part}"
            d = float(np.abs(got[s] - ref[s]).max())
            factor = (widened or {}).get((li, part), 1.0)
            if part == "biases" and li in bias_at_weight_scale:
                assert factor == 1.0, f"{name}: held at the weights' scale and widened"
                scale = max(1e-3, float(np.abs(ref[ws]).max()))
                allowance = rtol * scale + 1e-6
                print(f"{name}: max |d| = {d:.3e} at the weights' scale = {scale:.3e} (own: {float(np.abs(ref[bs]).max()):.3e}) rtol = {rtol} used = {d / allowance:.3f}")
                assert d <= allowance, (tag, li, d, scale, rtol)
            elif factor != 1.0:
                allowance = factor * (rtol * max(1e-3, float(np.abs(ref[s]).max())) + 1e-6)
                print(f"{name}: max |d| = {d:.3e} allowance x {factor:.3f} = {allowance:.3e} used = {d / allowance:.3f} (unwidened: {d * factor / allowance:.3f})")
                assert d <= allowance, (tag, li, part, d, allowance)
            else:
                worst = max(worst, close(got[s], ref[s], rtol, name))
                continue
            worst = max(worst, d / allowance)
    return worst
