"""The float64 torch twin of ("dwconv_linear",) = Conv2d(C, C, 3, padding=1, groups=C), for tests/test_convnet_dw_plan.py and
tests/test_gpu_convnet_dw.py.  `DwNet` is tests/_pw_ref.py's PwNet with that kind, so one twin covers all twelve kinds.  The flat layout
has a (9, C) block per depthwise layer (row t = 3 kh + kw), which none of the helper modules knows, so this module has its own
param_shapes / tensor_slices / n_logical / random_params, and `compare` / `close_per_tensor` run _twin_checks' and _torch_ref's own code
with _torch_ref.param_shapes routed here for the call (`layouts`, the routing of tests/_pw_ref.py).  The bounds are the stride file's,
re-exported through _pw_ref, nothing widened.  The nets of the GPU file, their seeds, options and the small-integer exact net are here,
so the CPU file prepares the twin's side from the same cases.
DwNet.__init__ lets PwNet.__init__ build the net from a stand-in description (every depthwise layer written as a square 1x1 layer with
zero parameters: the same maps, kinds, skips and statistics) and then puts the depthwise modules in; an attribute a base class gains is
inherited.  Folding the three subclasses into tests/_torch_ref.py is the follow-up the README names.
Not a test file: every assert carries its message."""
import contextlib

import numpy as np
import _pw_ref
import _torch_ref
import _twin_checks
from _pw_ref import PW, RTOL, RTOL_2, STEPS, PwNet, layout, layout_spec  # noqa: F401  (the bounds are the stride file's, re-exported)

DW = "dwconv_linear"


def separable(c):
    """a separable layer to c channels"""
    return ((DW,), ("bn_relu",), (PW, c), ("bn_relu",))


def residual(c):
    """a residual separable block behind a layer of c channels"""
    return ((DW,), ("bn_relu",), (PW, c), ("bn_add_relu", 4))


def param_shapes(in_shape, layers):
    """_pw_ref.param_shapes with the depthwise convolution: K = 9, Cout = C"""
    H, W, C = in_shape
    flat, out = False, []
    for l in layers:
        if l[0] in ("conv", "conv_linear"):
            out.append((9 * C, l[1])); C = l[1]
        elif l[0] == PW:
            assert not flat, "a 1x1 convolution behind the dense stage"
            out.append((C, l[1])); C = l[1]
        elif l[0] == DW:
            assert not flat, "a depthwise convolution behind the dense stage"
            assert len(l) == 1 or l[1] in (0, C), f"a depthwise layer of another width: {l}"
            out.append((9, C))
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
    """_twin_checks.compare, unchanged, on a description with the kind (kw: its unrounded_logits / widened_gradients)"""
    with layouts():
        return _twin_checks.compare(layout_spec(spec), r, ref, rtol, rtol2, steps, tag, **kw)


# (input shape, layers, batch): the smallest nets at which each thing can go wrong
# A: H != W, and with H = 3 every output row touches a border; a ReLU convolution below (epilogue 3 gated by its output)
W_A = ((3, 5, 3), (("conv", 32), (DW,), ("bn_relu",), ("global_avgpool",), ("dense", 7)), 3)
# B: C = 96 (three channel groups, 24 quads: no power of two, so a lane's quad is not tid % 24 in every tile and the kernel keys its weights by
# the quad -- but the row is 10 x 24 = 240 pieces, ONE slab, so no lane's quad ever changes here: tests/_kinds_cases.py's net "quads" has the
# second slab and runs the reload); M = 300: with pix_per_chunk = 128
# three weight-gradient chunks, the last partial, whose edges fall mid-row and mid-image; the skip's add behind the dw input gradient
W_B = ((6, 10, 3), (("conv_linear", 96), ("bn_relu",)) + residual(96) + (("pool",), ("global_avgpool",), ("dense", 10)), 5)
# C: the dw layer on a 2 x 2 map (every tap of every pixel but the centre's own meets a border); a pool below (epilogue 0, raw); a dense
# layer above a self-gated batch normalisation.  (The issue writes 8 x 8 with two pools; a pool behind a pool is refused, so 4 x 4 and one.)
W_C = ((4, 4, 3), (("conv", 32), ("pool",), (DW,), ("bn_relu",), ("dense_relu", 32), ("dense", 10)), 2)
# D: dw as layer 0 (no input gradient) and at C = 256 on a 10 x 18 map (the issue's 16 x 16 would be four whole slabs and two whole bands):
# a row holds 18 x 64 = 1152 pieces = 4.5 slabs of 256, and 10 rows are a band of 8 and one of 2 -- forward and gated input gradient span
# more than one tile in both tiled directions and are a multiple of the tile in neither; M = 1440: twelve weight-gradient chunks of 128 pixels, the last of 32
W_D = ((10, 18, 32), ((DW,), ("bn_relu",), (PW, 256), ("bn_relu",), (DW,), ("bn_relu",), ("global_avgpool",), ("dense", 10)), 8)
NETS = {"a": W_A, "b": W_B, "c": W_C, "d": W_D}
# the bf16_stored refusal: net c on an 8 x 8 input, whose convolution and pool the bf16-tensor kernels cover, so the refusal is batch normalisation's
W_S = ((8, 8, 3), (("conv", 32), ("pool",), (DW,), ("bn_relu",), ("dense_relu", 32), ("dense", 10)), 2)
OPTIONS = {"a": (), "b": (("pix_per_chunk", 128),), "c": (), "d": ()}
LOOPING = (("halo_f32_slots", 3),)          # net d once more: three workgroups over its 80 tiles

# per net the seeds of its parameters and of its batch, chosen from the twin alone: tests/test_convnet_dw_plan.py asserts the margin
# condition of _twin_checks.compare in both precisions and that the bf16-operand twin run in float32 agrees with itself in float64
SEEDS = {"a": (18, 19), "b": (0, 1), "c": (4, 5), "d": (6, 7)}


def case(name, seeds=None):
    """(parameters, x, y) of net `name` from its SEEDS (or from `seeds`).  Net d's logits layer carries the biases linspace(-4.5, 4.5), as
    _pw_ref's net d: its rows' features are means over 180 pixels and barely differ"""
    in_shape, layers, B = NETS[name]
    seeds = seeds or SEEDS[name]
    flat = random_params(np.random.default_rng(seeds[0]), in_shape, layers)
    if name == "d":
        flat[tensor_slices(in_shape, layers)[-1][1]] = np.linspace(-4.5, 4.5, layers[-1][1]).astype(np.float32)
    rng = np.random.default_rng(seeds[1])
    return flat, rng.standard_normal((B,) + in_shape).astype(np.float32), rng.integers(0, layers[-1][1], B).astype(np.int32)


def _unreversed(torch):
    """the depthwise convolution whose input gradient forgets to reverse the taps (a MUTANT): dX correlates dZ with W instead of flip(W)"""
    class Unreversed(torch.autograd.Function):
        @staticmethod
        def forward(ctx, x, w, b):
            ctx.save_for_backward(x, w)
            return torch.nn.functional.conv2d(x, w, b, padding=1, groups=x.shape[1])

        @staticmethod
        def backward(ctx, g):
            x, w = ctx.saved_tensors
            C = x.shape[1]
            return (torch.nn.grad.conv2d_input(x.shape, w.flip(2, 3), g, padding=1, groups=C), torch.nn.grad.conv2d_weight(x, w.shape, g, padding=1, groups=C), g.sum((0, 2, 3)))
    return Unreversed.apply


class DwNet(PwNet):
    """PwNet with ("dwconv_linear",).  self.kinds names it "conv_linear" (its module has groups = C), so the flat views are TorchNet's: a
    (C, 1, 3, 3) weight flattens to W[t = 3 kh + kw][c].  Its operands are never rounded: under operand = "bf16" the layer computes as under
    "f64", as the library computes it in fp32 in either mode.  PwNet's mutants reach the kind (drop_bias_grad: its bias too;
    open_gate_below: the ReLU below a depthwise layer too; drop_skip_share), and three more make MUTANTS, never a model of the library:
    taps_transposed -- W[kh][kw] applied as W[kw][kh]; taps_unreversed -- the input gradient correlates dZ with the taps as they stand;
    wrap_border -- the column left of the map is the map's last column instead of zeros (one border column treated as inside)."""

    def __init__(self, in_shape, layers, flat, taps_transposed=False, taps_unreversed=False, wrap_border=False, **kw):
        import torch
        layers = [tuple(l) for l in layers]
        flat = np.asarray(flat, dtype=np.float64)
        assert flat.size == n_logical(in_shape, layers), (flat.size, n_logical(in_shape, layers))
        shapes, slices = param_shapes(in_shape, layout(layers)), tensor_slices(in_shape, layers)
        with_params = [i for i, l in enumerate(layers) if l[0] not in _torch_ref.NO_PARAMS]
        stand, pieces = list(layers), []
        for i, (k, c), (ws, bs) in zip(with_params, shapes, slices):
            if layers[i][0] == DW:
                stand[i] = (PW, c)
                pieces.append(np.zeros(c * c + c))
            else:
                pieces.append(flat[ws.start:bs.stop])
        super().__init__(in_shape, tuple(stand), np.concatenate(pieces), **kw)
        self.res_layers = layers
        self.taps_unreversed, self.wrap_border = taps_unreversed, wrap_border
        for i, (k, c), (ws, bs) in zip(with_params, shapes, slices):
            if layers[i][0] != DW:
                continue
            m = torch.nn.Conv2d(c, c, 3, padding=1, groups=c).double()
            w = flat[ws].reshape(3, 3, c)                                   # W[kh][kw][c]
            if taps_transposed:
                w = w.transpose(1, 0, 2)
            with torch.no_grad():
                m.weight.copy_(torch.from_numpy(np.ascontiguousarray(w.transpose(2, 0, 1)[:, None])))      # weight[c, 0, kh, kw]
                m.bias.copy_(torch.from_numpy(flat[bs].copy()))
            self.mods[i] = m.float() if kw.get("arithmetic", "float64") == "float32" else m

    def _conv(self, m, t):
        """PwNet._conv; a depthwise module is applied unrounded whatever the operand mode"""
        if m.groups == 1:
            return super()._conv(m, t)
        F = self.torch.nn.functional
        bias = m.bias.detach() if self.drop_bias_grad else m.bias
        if self.taps_unreversed:
            return _unreversed(self.torch)(t, m.weight, bias)
        if self.wrap_border:
            left = F.pad(t[..., -1:], (0, 0, 1, 1))
            return F.conv2d(self.torch.cat([left, F.pad(t, (0, 1, 1, 1))], -1), m.weight, bias, groups=m.groups)
        return F.conv2d(t, m.weight, bias, padding=1, groups=m.groups)


# ---- exact data: a small-integer net whose forward sums are exact in every precision and every summation order ------------------------------
# 4 x 6 x 32 input of integers in -2 .. 2; a depthwise layer with weights in -1 .. 1 and biases in -3 .. 3 (|z| <= 21); batch normalisation
# in evaluation made the identity (exact_case); a second depthwise layer on the ReLU map (|z| <= 9 * 21 + 3 = 192: eight bits, exact as a
# bf16 operand of the dense layer); a dense layer on the flattened 4 x 6 x 32 map with weights in -1 .. 1 (|logit| <= 768 * 192 + 3 < 2^24).
X_SPEC = ((4, 6, 32), ((DW,), ("bn_relu",), (DW,), ("bn_relu",), ("dense", 5)), 3)


def _dw_int(x, W, b):
    """the depthwise convolution in int64: x[B][H][W][C], W[9][C], b[C]"""
    B, H, Wd, C = x.shape
    xp = np.zeros((B, H + 2, Wd + 2, C), dtype=np.int64)
    xp[:, 1:-1, 1:-1] = x
    z = np.zeros_like(x) + b
    for kh in range(3):
        for kw in range(3):
            z += W[3 * kh + kw] * xp[:, kh:kh + H, kw:kw + Wd]
    return z


def exact_case(seed=0, spec=X_SPEC):
    """(parameters, running statistics, x, the integer logits by NumPy int64, the second map) of X_SPEC (or of `spec`: the same five layers
    on another map and batch) under evaluation, the batch normalisation layers made the identity as _pw_ref.exact_case makes them"""
    in_shape, layers, B = spec
    assert tuple(tuple(l) for l in layers) == X_SPEC[1] and in_shape[0] * in_shape[1] * in_shape[2] * 192 + 3 < 2 ** 24, spec
    rng = np.random.default_rng(seed)
    H, W, C = in_shape
    x = rng.integers(-2, 3, (B, H, W, C)).astype(np.int64)
    W1, b1 = rng.integers(-1, 2, (9, C)).astype(np.int64), rng.integers(-3, 4, C).astype(np.int64)
    W2, b2 = rng.integers(-1, 2, (9, C)).astype(np.int64), rng.integers(-3, 4, C).astype(np.int64)
    W3, b3 = rng.integers(-1, 2, (H * W * C, 5)).astype(np.int64), rng.integers(-3, 4, 5).astype(np.int64)
    a1 = np.maximum(0, _dw_int(x, W1, b1))
    a2 = np.maximum(0, _dw_int(a1, W2, b2))
    assert a1.max() <= 21 and a2.max() <= 255, (a1.max(), a2.max())
    logits = a2.reshape(B, -1) @ W3 + b3
    flat = np.concatenate([W1.ravel(), b1, np.ones(C), np.zeros(C), W2.ravel(), b2, np.ones(C), np.zeros(C), W3.ravel(), b3]).astype(np.float32)
    eps = float(np.float32(1e-5))
    var = np.float32(1.0 - eps)
    assert np.float32(1.0 / np.sqrt(float(var) + eps)) == np.float32(1.0), "fl32(1 / sqrt(var + eps)), the library's invstd, must be 1.0f"
    stats = np.concatenate([np.zeros(C), np.full(C, var), np.zeros(C), np.full(C, var)]).astype(np.float32)
    return flat, stats, x.astype(np.float32), logits, a2


def against_torch(spec, configure, make_optim, micro=1, rtol=4e-4, tag="", ema=0.0):
    """_pw_ref.against_torch for a net with the kind: ONE update of `micro` micro-batches on the device and on the DwNet twin"""
    from _convnet_util import close, dev, make_net, same_bits, step
    in_shape, layers, B = spec
    with layouts():
        flat, data = _twin_checks.update_case(layout_spec(spec), micro)
    net = make_net(spec, "fp32")
    net.set_params(flat)
    configure(net)
    if ema:
        net.set_ema(ema)
    ref = DwNet(in_shape, layers, flat)
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
