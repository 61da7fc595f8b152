"""The reference of the residual-block tests: tests/_bn_ref.py's float64 torch twin with ("bn_add_relu", d) layers,
y = relu(BatchNorm2d(z) + s), s the output of the layer d places in front (torchvision's BasicBlock with an identity shortcut).  A
bn_add_relu layer owns what a bn_relu layer owns -- one K = 1 block [gamma | beta] and running statistics -- so the flat layouts are those
of the description with every ("bn_add_relu", d) written ("bn_relu",): `plain`.  Not a test file: every assert carries its message."""
import _bn_ref
from _bn_ref import TorchNet, close  # noqa: F401  (close: for the test files)


def plain(layers):
    """the description with every ("bn_add_relu", d) written ("bn_relu",): the same parameters, statistics and flat layouts, no skip"""
    return tuple(("bn_relu",) if l[0] == "bn_add_relu" else tuple(l) for l in layers)


def skips(layers):
    """{index of a bn_add_relu layer: index of its source}"""
    return {i: i - l[1] for i, l in enumerate(layers) if l[0] == "bn_add_relu"}


def param_shapes(in_shape, layers):
    return _bn_ref.param_shapes(in_shape, plain(layers))


def tensor_slices(in_shape, layers):
    return _bn_ref.tensor_slices(in_shape, plain(layers))


def n_logical(in_shape, layers):
    return _bn_ref.n_logical(in_shape, plain(layers))


def random_params(rng, in_shape, layers):
    return _bn_ref.random_params(rng, in_shape, plain(layers))


def close_per_tensor(got, ref, in_shape, layers, rtol, tag="", bias_at_weight_scale=()):
    return _bn_ref.close_per_tensor(got, ref, in_shape, plain(layers), rtol, tag, bias_at_weight_scale)


class ResTorchNet(TorchNet):
    """TorchNet of a description with bn_add_relu layers.  forward remembers every layer's output (self.outs, tensors in the graph) and adds
    the source's in front of a bn_add_relu layer's ReLU.  gate_source = False DROPS the ReLU of every skip source on the skip path only
    (the skip then carries the source's pre-activation): what a backward pass without the source gate computes the gradient of -- for the
    gate-swap test, never a model of the library."""

    def __init__(self, in_shape, layers, flat, momentum=0.1, eps=1e-5, operand="f64", gate_source=True):
        super().__init__(in_shape, plain(layers), flat, momentum, eps, operand)
        self.skips, self.gate_source = skips(layers), gate_source
        self.res_layers = [tuple(l) for l in layers]
        for i, s in self.skips.items():
            assert 0 <= s < i - 1 and self.kinds[i - 1] == "conv_linear", (i, s, self.kinds)
        self.outs = []

    def forward(self, x, train):
        torch = self.torch
        import numpy as np
        self._mode(train)
        t = torch.from_numpy(np.ascontiguousarray(np.asarray(x, dtype=np.float64).transpose(0, 3, 1, 2)))
        self.outs, pre = [], []
        for i, (kind, m) in enumerate(zip(self.kinds, self.mods)):
            if kind in ("dense", "dense_relu") and t.dim() == 4:
                t = t.permute(0, 2, 3, 1).reshape(t.shape[0], -1)          # NHWC flatten
            t = self._rounded(m, t) if self.operand == "bf16" and self._is_rounded(kind, m) else m(t)
            if i in self.skips:
                s = self.skips[i]
                if self.gate_source:
                    t = t + self.outs[s]
                else:
                    # the same VALUE as the gated sum, but the gradient of the skip path passes the source's ReLU as if it were open
                    t = t + (self.outs[s].detach() + pre[s] - pre[s].detach())
            pre.append(t)
            if kind in ("conv", "bn_relu", "dense_relu"):
                t = torch.relu(t)
            self.outs.append(t)
        return t
