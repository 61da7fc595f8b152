"""The float64 torch twin of ("dwconv_linear_s2",) = Conv2d(C, C, 3, stride=2, padding=1, groups=C), ("bn",) = BatchNorm2d(C) with no
activation and ("bn_add", d) = BatchNorm2d(z) + s with none, for tests/test_convnet_mb_plan.py and tests/test_gpu_convnet_mb.py.  `MbNet`
is tests/_dw_ref.py's DwNet with those kinds, so one twin covers all fifteen.  As in _dw_ref.py this module has its own param_shapes /
tensor_slices / n_logical / random_params walk (a strided depthwise layer is a (9, C) block AND halves the map, which no helper module
knows), and `compare` / `close_per_tensor` run _twin_checks' and _torch_ref's own code with _torch_ref.param_shapes routed here for the
call (`layouts`).  The bounds are the stride file's, re-exported through _pw_ref and _dw_ref, nothing widened.  The nets of the GPU file,
their seeds, options and the small-integer exact net are here, so the CPU file prepares the twin's side from the same cases.
MbNet.__init__ lets DwNet.__init__ build the net from a stand-in description -- a strided depthwise layer written as a dense strided 3x3
layer C -> C with zero parameters (the same halved map), "bn" as "bn_relu", ("bn_add", d) as ("bn_add_relu", d): the same maps, skips and
statistics -- and then puts the strided depthwise modules in and remembers which batch-normalisation layers have no ReLU.  Folding the
four subclasses into tests/_torch_ref.py is the follow-up the README names.
Not a test file: every assert carries its message."""
import contextlib

import numpy as np
import _torch_ref
import _twin_checks
from _dw_ref import DW, PW, RTOL, RTOL_2, STEPS, DwNet  # noqa: F401  (the bounds are the stride file's, re-exported)
from _pw_ref import layout as _pw_layout

DWS2, BN, BNA = "dwconv_linear_s2", "bn", "bn_add"
BN_KINDS = ("bn_relu", "bn_add_relu", "bn_add_relu_down", BN, BNA)


def inverted(c, t=2):
    """an inverted residual block of expansion t behind a layer of c channels (identity skip, no activation behind the sum)"""
    return ((PW, t * c), ("bn_relu",), (DW,), ("bn_relu",), (PW, c), (BNA, 6))


def inverted_s2(c, co, t=2):
    """an inverted residual block that halves the map and goes from c to co channels (no skip, no activation behind the projection)"""
    return ((PW, t * c), ("bn_relu",), (DWS2,), ("bn_relu",), (PW, co), (BN,))


def layout(layers):
    """the description in the kinds the flat views know: _pw_ref.layout, and either linear batch-normalisation kind a bn_relu (the same
    [gamma | beta] block and statistics); both depthwise kinds keep theirs (param_shapes below)"""
    return tuple(("bn_relu",) if l[0] in (BN, BNA) else l for l in _pw_layout(layers))


def layout_spec(spec):
    return (spec[0], layout(spec[1]), spec[2])


def param_shapes(in_shape, layers):
    """_dw_ref.param_shapes with the strided depthwise convolution: K = 9, Cout = C, and the map halves"""
    H, W, C = in_shape
    flat, out = False, []
    for l in layers:
        if l[0] in ("conv", "conv_linear"):
            out.append((9 * C, l[1])); C = l[1]
        elif l[0] == PW:
            assert not flat, "a 1x1 convolution behind the dense stage"
            out.append((C, l[1])); C = l[1]
        elif l[0] in (DW, DWS2):
            assert not flat, "a depthwise convolution behind the dense stage"
            assert len(l) == 1 or l[1] in (0, C), f"a depthwise layer of another width: {l}"
            out.append((9, C))
            if l[0] == DWS2:
                assert H % 2 == 0 and W % 2 == 0, (H, W)
                H, W = H // 2, W // 2
        elif l[0] in BN_KINDS:
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
    slices, o = [], 0
    for k, c in param_shapes(in_shape, layout(layers)):
        slices.append((slice(o, o + k * c), slice(o + k * c, o + k * c + c)))
        o += k * c + c
    return slices


def n_logical(in_shape, layers):
    return tensor_slices(in_shape, layers)[-1][1].stop


@contextlib.contextmanager
def layouts():
    """_torch_ref's flat views (tensor_slices, n_logical, random_params, close_per_tensor) with this module's param_shapes, for one call"""
    old = _torch_ref.param_shapes
    _torch_ref.param_shapes = param_shapes
    try:
        yield
    finally:
        _torch_ref.param_shapes = old


def random_params(rng, in_shape, layers):
    with layouts():
        return _torch_ref.random_params(rng, in_shape, layout(layers))


def close_per_tensor(got, ref, in_shape, layers, rtol, tag=""):
    with layouts():
        return _torch_ref.close_per_tensor(got, ref, in_shape, layout(layers), rtol, tag)


def compare(spec, r, ref, rtol, rtol2, steps, tag, **kw):
    """_twin_checks.compare, unchanged, on a description with the kinds"""
    with layouts():
        return _twin_checks.compare(layout_spec(spec), r, ref, rtol, rtol2, steps, tag, **kw)


# (input shape, layers, batch): the smallest nets at which each thing can go wrong
# A: H != W and a 2 x 3 output: output row 0 at the top border, row 1 on the input row that row 0 kept, every column step of the window;
# a ReLU convolution below (the input gradient's epilogue 3, gated by its output)
M_A = ((4, 6, 3), (("conv", 32), (DWS2,), ("bn_relu",), ("global_avgpool",), ("dense", 7)), 3)
# B: the strided layer on a 2 x 2 map -> 1 x 1 (one output pixel, five of its nine taps outside the map), above a pool (epilogue 0, raw);
# BH: H = 2 with W = 8 (one output row, the window never slides); BW: W = 2 with H = 8 (one output column, every block at the right edge
# of dZ).  Six samples: batch normalisation over a 1 x 1 map has B rows.
_B_TAIL = ((DWS2,), ("bn_relu",), ("dense_relu", 32), ("dense", 10))
M_B = ((4, 4, 3), (("conv", 32), ("pool",)) + _B_TAIL, 6)
M_BH = ((4, 16, 3), (("conv", 32), ("pool",)) + _B_TAIL, 6)
M_BW = ((16, 4, 3), (("conv", 32), ("pool",)) + _B_TAIL, 6)
# C: C = 96 (24 quads, three channel groups) on 12 x 20 -> 6 x 10, B = 5: M_out = 300, with pix_per_chunk = 128 three weight-gradient
# chunks, the last of 44, whose edges fall mid-row and mid-image; a bn_relu below (epilogue 3)
M_C = ((12, 20, 3), (("conv_linear", 96), ("bn_relu",), (DWS2,), ("bn_relu",), ("global_avgpool",), ("dense", 10)), 5)
# D: the strided layer as layer 0 on 32 channels (no input gradient; 40 x 72 -> 20 x 36: three bands of 8 output rows, 288 pieces = two
# slabs) and at C = 256 on 20 x 36 -> 10 x 18, B = 8: a band of 8 and one of 2, 18 x 64 = 1152 pieces = 4.5 slabs -- forward and gated
# input gradient span several tiles in both directions and are a multiple of the tile in neither; M_out = 1440: twelve chunks, the last of 32
M_D = ((40, 72, 32), ((DWS2,), ("bn_relu",), (PW, 256), ("bn_relu",), (DWS2,), ("bn_relu",), ("global_avgpool",), ("dense", 10)), 8)
# E: two inverted residual blocks back to back at widths 32 -> (64) -> 32 on 6 x 10 -- the first bn_add from a bn_relu source (layer 1),
# the second from the first bn_add (layer 7) -- then a strided block ending in bn, a 1x1 layer, bn_relu, gap, dense: the whole gating
# table of the linear kinds in one net
M_E = ((6, 10, 3), (("conv_linear", 32), ("bn_relu",)) + inverted(32) + inverted(32) + inverted_s2(32, 32) + ((PW, 64), ("bn_relu",), ("global_avgpool",), ("dense", 10)), 4)
# F: bn_add from a pool source (layer 1); bn_add directly below a ReLU convolution; bn directly below a ReLU convolution and below a
# stride-1 depthwise layer
M_F = ((8, 8, 3), (("conv", 32), ("pool",)) + inverted(32) + (("conv", 32), (PW, 32), (BN,), ("conv", 32), (PW, 32), (BN,), (DW,), ("bn_relu",), ("global_avgpool",), ("dense", 10)), 4)
NETS = {"a": M_A, "b": M_B, "bh": M_BH, "bw": M_BW, "c": M_C, "d": M_D, "e": M_E, "f": M_F}
# the bf16_stored refusal: net b on an 8 x 8 input, whose convolution and pool the bf16-tensor kernels cover, so the refusal is batch normalisation's
M_S = ((8, 8, 3), (("conv", 32), ("pool",)) + _B_TAIL, 2)
OPTIONS = {n: () for n in NETS}
OPTIONS["c"] = (("pix_per_chunk", 128),)
LOOPING = (("halo_f32_slots", 3),)          # net d once more: three workgroups over its tiles

# per net the seeds of its parameters and of its batch, chosen from the twin alone: tests/test_convnet_mb_plan.py asserts the margin
# condition of _twin_checks.compare in both precisions and that the bf16-operand twin run in float32 agrees with itself in float64
SEEDS = {"a": (6, 7), "b": (0, 1), "bh": (14, 15), "bw": (20, 21), "c": (2, 3), "d": (8, 9), "e": (30, 31), "f": (4, 5)}


def case(name, seeds=None):
    """(parameters, x, y) of net `name` from its SEEDS (or from `seeds`).  Net d's logits layer carries the biases linspace(-4.5, 4.5), as
    _dw_ref's net d: its rows' features are means over 180 pixels and barely differ"""
    in_shape, layers, B = NETS[name]
    seeds = seeds or SEEDS[name]
    flat = random_params(np.random.default_rng(seeds[0]), in_shape, layers)
    if name == "d":
        flat[tensor_slices(in_shape, layers)[-1][1]] = np.linspace(-4.5, 4.5, layers[-1][1]).astype(np.float32)
    rng = np.random.default_rng(seeds[1])
    return flat, rng.standard_normal((B,) + in_shape).astype(np.float32), rng.integers(0, layers[-1][1], B).astype(np.int32)


def _unreversed_s2(torch):
    """the strided depthwise convolution whose input gradient forgets to reverse the taps (a MUTANT): dX is built from flip(W), which for a
    correlation's transpose means dZ meets the taps as they stand"""
    class Unreversed(torch.autograd.Function):
        @staticmethod
        def forward(ctx, x, w, b):
            ctx.save_for_backward(x, w)
            return torch.nn.functional.conv2d(x, w, b, stride=2, padding=1, groups=x.shape[1])

        @staticmethod
        def backward(ctx, g):
            x, w = ctx.saved_tensors
            C = x.shape[1]
            return (torch.nn.grad.conv2d_input(x.shape, w.flip(2, 3), g, stride=2, padding=1, groups=C),
                    torch.nn.grad.conv2d_weight(x, w.shape, g, stride=2, padding=1, groups=C), g.sum((0, 2, 3)))
    return Unreversed.apply


def _gate_gradient(torch, t):
    """t's value, with the gradient passing only where t > 0: what a backward pass that gates a tensor without a ReLU computes"""
    r = torch.relu(t)
    return t.detach() + r - r.detach()


class MbNet(DwNet):
    """DwNet with ("dwconv_linear_s2",), ("bn",) and ("bn_add", d).  self.kinds names the strided depthwise layer "conv_linear" (its module
    has groups = C and stride 2) and either linear batch normalisation "bn_relu", so the flat views are TorchNet's; self.linear holds the
    layers whose ReLU forward() leaves out.  The strided depthwise module is never rounded: under operand = "bf16" it computes as under
    "f64", as the library computes it in fp32 in either mode.  DwNet's and PwNet's mutants reach the kinds (drop_skip_share: a bn_add's
    skip too; taps_transposed / taps_unreversed: the strided layer too), and four more make MUTANTS, never a model of the library:
    phase_off -- the stencil reads rows 2i + kh and columns 2j + kw (for 2i + kh - 1, 2j + kw - 1); relu_in_bn -- a ReLU applied behind
    every linear batch normalisation; gate_linear -- the gradient of a linear batch normalisation's output gated with out > 0 (same
    values); gate_linear_source -- the skip's share gated by the output of a source that is a linear batch normalisation."""

    def __init__(self, in_shape, layers, flat, phase_off=False, relu_in_bn=False, gate_linear=False, gate_linear_source=False, **kw):
        import torch
        layers = [tuple(l) for l in layers]
        flat = np.asarray(flat, dtype=np.float64)
        assert flat.size == n_logical(in_shape, layers), (flat.size, n_logical(in_shape, layers))
        shapes, slices = param_shapes(in_shape, layout(layers)), tensor_slices(in_shape, layers)
        with_params = [i for i, l in enumerate(layers) if l[0] not in _torch_ref.NO_PARAMS]
        stand = [("bn_relu",) if l[0] == BN else ("bn_add_relu", l[1]) if l[0] == BNA else l for l in layers]
        pieces = []
        for i, (k, c), (ws, bs) in zip(with_params, shapes, slices):
            if layers[i][0] == DWS2:
                stand[i] = ("conv_linear_s2", c)
                pieces.append(np.zeros(9 * c * c + c))
            else:
                pieces.append(flat[ws.start:bs.stop])
        super().__init__(in_shape, tuple(stand), np.concatenate(pieces), **kw)
        self.res_layers = layers
        self.linear = {i for i, l in enumerate(layers) if l[0] in (BN, BNA)}
        self.phase_off, self.relu_in_bn, self.gate_linear, self.gate_linear_source = phase_off, relu_in_bn, gate_linear, gate_linear_source
        transposed = kw.get("taps_transposed", False)
        for i, (k, c), (ws, bs) in zip(with_params, shapes, slices):
            if layers[i][0] != DWS2:
                continue
            m = torch.nn.Conv2d(c, c, 3, stride=2, padding=1, groups=c).double()
            w = flat[ws].reshape(3, 3, c)                                   # W[kh][kw][c]
            if transposed:
                w = w.transpose(1, 0, 2)
            with torch.no_grad():
                m.weight.copy_(torch.from_numpy(np.ascontiguousarray(w.transpose(2, 0, 1)[:, None])))      # weight[c, 0, kh, kw]
                m.bias.copy_(torch.from_numpy(flat[bs].copy()))
            self.mods[i] = m.float() if kw.get("arithmetic", "float64") == "float32" else m

    def _conv(self, m, t):
        """DwNet._conv; a strided depthwise module is applied unrounded whatever the operand mode"""
        if m.groups == 1 or m.stride != (2, 2):
            return super()._conv(m, t)
        F = self.torch.nn.functional
        bias = m.bias.detach() if self.drop_bias_grad else m.bias
        if self.taps_unreversed:
            return _unreversed_s2(self.torch)(t, m.weight, bias)
        if self.phase_off:
            return F.conv2d(F.pad(t, (0, 1, 0, 1)), m.weight, bias, stride=2, groups=m.groups)
        return F.conv2d(t, m.weight, bias, stride=2, padding=1, groups=m.groups)

    def forward(self, x, train):
        """PwNet.forward without the ReLU behind a linear batch normalisation, and with the mutants of the linear kinds"""
        torch = self.torch
        self._mode(train)
        t = torch.from_numpy(np.ascontiguousarray(np.asarray(x, dtype=self.np_dtype).transpose(0, 3, 1, 2)))
        self.outs, pre = [], []
        for i, (kind, m) in enumerate(zip(self.kinds, self.mods)):
            if kind in ("dense", "dense_relu") and t.dim() == 4:
                t = t.permute(0, 2, 3, 1).reshape(t.shape[0], -1)          # NHWC flatten
            if kind == "global_avgpool":
                t = t.mean((2, 3))
            elif kind in ("conv", "conv_linear"):
                t = self._conv(m, t)
            else:
                t = self._rounded(m, t) if self.operand == "bf16" and self._is_rounded(kind, m) else m(t)
            if i in self.skips:
                s = self.skips[i]
                src = self.outs[s]
                if self.gate_linear_source and s in self.linear:
                    src = _gate_gradient(torch, src)
                src = src.detach() if self.drop_skip_share else src
                t = t + (self._shortcut(src, t.shape[1]) if i in self.down else src)
            pre.append(t)
            if i in self.linear:
                if self.relu_in_bn:
                    t = torch.relu(t)
                elif self.gate_linear:
                    t = _gate_gradient(torch, t)
            elif kind in ("conv", "bn_relu", "dense_relu"):
                r = torch.relu(t)
                t = r.detach() + t - t.detach() if self.open_gate_below and i in self.below_pw else r
            self.outs.append(t)
        return t


# ---- exact data: a small-integer net whose forward sums are exact in every precision and every summation order ------------------------------
# 8 x 12 x 32 input of integers in -2 .. 2; a strided depthwise layer with weights in -1 .. 1 and biases in -3 .. 3 (|z| <= 21) onto
# 4 x 6; a linear batch normalisation in evaluation made the identity (negative values pass: no ReLU); a stride-1 depthwise layer on that
# map (|z| <= 9 * 21 + 3 = 192); bn_relu made the identity in front of its ReLU (eight bits, exact as a bf16 operand of the dense layer);
# a dense layer on the flattened 4 x 6 x 32 map with weights in -1 .. 1 (|logit| <= 768 * 192 + 3 < 2^24).
X_SPEC = ((8, 12, 32), ((DWS2,), (BN,), (DW,), ("bn_relu",), ("dense", 5)), 3)


def _dw_int(x, W, b, stride):
    """the depthwise convolution in int64: x[B][H][W][C], W[9][C], b[C], padding 1"""
    B, H, Wd, C = x.shape
    xp = np.zeros((B, H + 2, Wd + 2, C), dtype=np.int64)
    xp[:, 1:-1, 1:-1] = x
    z = np.zeros((B, H, Wd, C), dtype=np.int64) + b
    for kh in range(3):
        for kw in range(3):
            z += W[3 * kh + kw] * xp[:, kh:kh + H, kw:kw + Wd]
    return z[:, ::stride, ::stride]


def exact_case(seed=0):
    """(parameters, running statistics, x, the integer logits by NumPy int64, the first and second maps) of X_SPEC under evaluation, both
    batch-normalisation layers made the identity as _dw_ref.exact_case makes them"""
    in_shape, layers, B = X_SPEC
    rng = np.random.default_rng(seed)
    H, W, C = in_shape
    x = rng.integers(-2, 3, (B, H, W, C)).astype(np.int64)
    W1, b1 = rng.integers(-1, 2, (9, C)).astype(np.int64), rng.integers(-3, 4, C).astype(np.int64)
    W2, b2 = rng.integers(-1, 2, (9, C)).astype(np.int64), rng.integers(-3, 4, C).astype(np.int64)
    K = (H // 2) * (W // 2) * C
    W3, b3 = rng.integers(-1, 2, (K, 5)).astype(np.int64), rng.integers(-3, 4, 5).astype(np.int64)
    a1 = _dw_int(x, W1, b1, 2)                                  # no ReLU: the linear batch normalisation is the identity
    a2 = np.maximum(0, _dw_int(a1, W2, b2, 1))
    assert np.abs(a1).max() <= 21 and a2.max() <= 255 and K * 192 + 3 < 2 ** 24, (np.abs(a1).max(), a2.max())
    logits = a2.reshape(B, -1) @ W3 + b3
    flat = np.concatenate([W1.ravel(), b1, np.ones(C), np.zeros(C), W2.ravel(), b2, np.ones(C), np.zeros(C), W3.ravel(), b3]).astype(np.float32)
    eps = float(np.float32(1e-5))
    var = np.float32(1.0 - eps)
    assert np.float32(1.0 / np.sqrt(float(var) + eps)) == np.float32(1.0), "fl32(1 / sqrt(var + eps)), the library's invstd, must be 1.0f"
    stats = np.concatenate([np.zeros(C), np.full(C, var), np.zeros(C), np.full(C, var)]).astype(np.float32)
    return flat, stats, x.astype(np.float32), logits, a1, a2


def against_torch(spec, configure, make_optim, micro=1, rtol=4e-4, tag="", ema=0.0):
    """_dw_ref.against_torch for a net with the kinds: ONE update of `micro` micro-batches on the device and on the MbNet twin"""
    from _convnet_util import close, dev, make_net, same_bits, step
    in_shape, layers, B = spec
    with layouts():
        flat, data = _twin_checks.update_case(layout_spec(spec), micro)
    net = make_net(spec, "fp32")
    net.set_params(flat)
    configure(net)
    if ema:
        net.set_ema(ema)
    ref = MbNet(in_shape, layers, flat)
    lr = _twin_checks.twin_update(ref, data, make_optim)
    for x, y in data:
        step(net, dev(net, x), dev(net, y), lr)
    assert not same_bits(net.get_params(), flat), f"{tag}: the update changed nothing"
    worst = close_per_tensor(net.get_params(), ref.params(), in_shape, layers, rtol, f"{tag} parameters")
    worst = max(worst, close(net.get_bn_stats(), ref.bn_stats(), rtol, f"{tag} running statistics"))
    if ema:
        e0 = flat.astype(np.float64)
        worst = max(worst, close_per_tensor(net.get_ema(), e0 + (1.0 - ema) * (ref.params() - e0), in_shape, layers, rtol, f"{tag} average"))
    print(f"{tag}: worst share of an allowance = {worst:.3f}")
    net.close()
    return worst
