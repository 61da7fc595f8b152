"""The float64 torch twin of ("conv1x1_linear", Cout) = Conv2d(Cin, Cout, 1), for tests/test_convnet_pw_plan.py and
tests/test_gpu_convnet_pw.py.  `PwNet` is tests/_stride_ref.py's StrideNet with that kind, so one twin covers all eleven kinds.  The flat
layout of a K = Cin block on a map is not expressible in kinds tests/_torch_ref.py knows (its dense layer has K = H W C), so this module
has its own param_shapes / tensor_slices / n_logical / random_params for descriptions with the kind, and `compare` / `close_per_tensor`
run _twin_checks' and _torch_ref's own code with _torch_ref.param_shapes routed here for the call (`layouts`).  The nets of the GPU file,
their seeds and the small-integer exact net are here, so the CPU file prepares the twin's side from the same cases.
Two stop-gaps until the kind is folded into tests/_torch_ref.py (the follow-up the README names), and what they depend on:
`layouts()` rebinds the module global _torch_ref.param_shapes for the length of one call, which works because tensor_slices, n_logical,
random_params and close_per_tensor all reach the shape walk through that one name; and PwNet.__init__ builds the net itself instead of
calling StrideNet.__init__ (which cannot build a 1x1 module), so it MIRRORS the attributes the base classes' methods read --
TorchNet's torch, in_shape, layers, res_layers, skips, mods, kinds, outs, gap_at, operand, gate_source, gate_below and StrideNet's np_dtype,
down, pad_other_side, sample_odd, lo_zero.  An attribute added to either base class has to be added there too.
Not a test file: every assert carries its message."""
import contextlib

import numpy as np
import _torch_ref
import _twin_checks
from _stride_ref import RTOL, RTOL_2, STEPS, StrideNet, _bf16t  # noqa: F401  (the bounds are the stride file's, re-exported)
from _torch_ref import NO_PARAMS

PW = "conv1x1_linear"


def bottleneck(c):
    """a bottleneck block of width c behind a layer of c channels"""
    return ((PW, c // 4), ("bn_relu",), ("conv_linear", c // 4), ("bn_relu",), (PW, c), ("bn_add_relu", 6))


def layout(layers):
    """the description in the kinds the flat views know: both skip kinds are a bn_relu, a strided convolution a conv_linear with a pool
    behind it (_stride_ref.layout); a 1x1 convolution keeps its kind (param_shapes below)"""
    out = []
    for l in layers:
        if l[0] == "conv_linear_s2":
            out += [("conv_linear", l[1]), ("pool",)]
        elif l[0] in ("bn_add_relu", "bn_add_relu_down"):
            out.append(("bn_relu",))
        else:
            out.append(tuple(l))
    return tuple(out)


def layout_spec(spec):
    return (spec[0], layout(spec[1]), spec[2])


def param_shapes(in_shape, layers):
    """_torch_ref.param_shapes with the 1x1 convolution: K = Cin on the map"""
    H, W, C = in_shape
    flat, out = False, []
    for l in layers:
        if l[0] in ("conv", "conv_linear"):
            out.append((9 * C, l[1])); C = l[1]
        elif l[0] == PW:
            assert not flat, "a 1x1 convolution behind the dense stage"
            out.append((C, l[1])); C = l[1]
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


def compare(spec, r, ref, rtol, rtol2, steps, tag):
    """_twin_checks.compare, unchanged, on a description with the kind"""
    with layouts():
        return _twin_checks.compare(layout_spec(spec), r, ref, rtol, rtol2, steps, tag)


# (input shape, layers, batch): the smallest nets at which each thing can go wrong
# A: M = 72, one partial row block; a ReLU convolution below (epilogue 3 gated by its output); H != W
P_A = ((4, 6, 3), (("conv", 32), (PW, 64), ("bn_relu",), ("global_avgpool",), ("dense", 7)), 3)
# B: M = 300, full and partial blocks; the skip's share added behind the 1x1 input gradient; 128 -> 32 and 32 -> 128
P_B = ((6, 10, 3), (("conv_linear", 128), ("bn_relu",)) + bottleneck(128) + (("pool",), ("global_avgpool",), ("dense", 10)), 5)
# C: M = 32, fewer rows than one block; a pool below (epilogue 0, raw); a dense layer above a self-gated batch normalisation
P_C = ((8, 8, 3), (("conv", 32), ("pool",), (PW, 128), ("bn_relu",), ("dense_relu", 32), ("dense", 10)), 2)
# D: layer 0 with no input gradient; K = 256 (eight K-tiles); its 256 -> 256 layer does not fit one slice in either precision: four column
# slices in fp32, two in bf16, forward and input gradient (the issue's 256 -> 64 fits the fp32 slice exactly and would be read once: widened
# to 256 to reach the multi-pass form); with pw = 0 the split-K form of the implicit GEMM; M = 2048, sixteen row blocks: with
# halo_f32_slots = 3 a workgroup takes several
P_D = ((16, 16, 32), ((PW, 256), ("bn_relu",), (PW, 256), ("bn_relu",), ("global_avgpool",), ("dense", 10)), 8)
NETS = {"a": P_A, "b": P_B, "c": P_C, "d": P_D}
# per net the options of its device run beside "pw": B's weight gradient in three chunks of 128 pixels, the last partial
OPTIONS = {"a": (), "b": (("pix_per_chunk", 128),), "c": (), "d": ()}
LOOPING = (("halo_f32_slots", 3),)          # net d once more: three workgroups (per column slice) over sixteen row blocks

# per net the seeds of its parameters and of its batch, chosen from the twin alone: tests/test_convnet_pw_plan.py asserts the margin
# condition of _twin_checks.compare in both precisions and that the bf16-operand twin run in float32 agrees with itself in float64
SEEDS = {"a": (0, 1), "b": (4, 5), "c": (0, 1), "d": (2, 3)}


def case(name, seeds=None):
    """(parameters, x, y) of net `name` from its SEEDS (or from `seeds`).  Net d's logits layer carries the biases linspace(-4.5, 4.5), as
    _stride_ref's net d: its rows' features are means over 256 pixels and barely differ"""
    in_shape, layers, B = NETS[name]
    seeds = seeds or SEEDS[name]
    flat = random_params(np.random.default_rng(seeds[0]), in_shape, layers)
    if name == "d":
        flat[tensor_slices(in_shape, layers)[-1][1]] = np.linspace(-4.5, 4.5, layers[-1][1]).astype(np.float32)
    rng = np.random.default_rng(seeds[1])
    return flat, rng.standard_normal((B,) + in_shape).astype(np.float32), rng.integers(0, layers[-1][1], B).astype(np.int32)


def _rounded_1x1(torch):
    """conv2d with a 1x1 filter on operands rounded to bfloat16, forward and backward, in the operands' own dtype: the forward rounds x and
    W, the input gradient dZ and W, the weight gradient x and dZ; the bias gradient sums dZ as it is"""
    class Rounded(torch.autograd.Function):
        @staticmethod
        def forward(ctx, x, w, b):
            xr, wr = _bf16t(x), _bf16t(w)
            ctx.save_for_backward(xr, wr)
            return torch.nn.functional.conv2d(xr, wr, b)

        @staticmethod
        def backward(ctx, g):
            xr, wr = ctx.saved_tensors
            gr = _bf16t(g)
            return torch.nn.grad.conv2d_input(xr.shape, wr, gr), torch.nn.grad.conv2d_weight(xr, wr.shape, gr), g.sum((0, 2, 3))
    return Rounded.apply


class PwNet(StrideNet):
    """StrideNet with ("conv1x1_linear", Cout).  self.kinds names it "conv_linear" (its module has a 1x1 filter), so the flat views are
    TorchNet's.  Four options make MUTANTS, never a model of the library: w_transposed -- the 1x1 layers apply W^T (square layers only);
    drop_bias_grad -- their bias gets no gradient; open_gate_below -- the ReLU of the layer directly below a 1x1 layer passes the gradient
    as if it were open; drop_skip_share -- the skip's share of the source's gradient is dropped."""

    def __init__(self, in_shape, layers, flat, momentum=0.1, eps=1e-5, operand="f64", arithmetic="float64", w_transposed=False, drop_bias_grad=False,
                 open_gate_below=False, drop_skip_share=False):
        import torch
        assert arithmetic in ("float64", "float32"), arithmetic
        self.np_dtype = np.float64 if arithmetic == "float64" else np.float32
        self.operand, self.gate_source, self.gate_below = operand, True, True
        self.pad_other_side = self.sample_odd = self.lo_zero = False
        self.w_transposed, self.drop_bias_grad, self.open_gate_below, self.drop_skip_share = w_transposed, drop_bias_grad, open_gate_below, drop_skip_share
        self.torch, self.in_shape = torch, tuple(in_shape)
        self.res_layers = [tuple(l) for l in layers]
        self.skips = {i: i - l[1] for i, l in enumerate(layers) if l[0] in ("bn_add_relu", "bn_add_relu_down")}
        self.down = {i: i - l[1] for i, l in enumerate(layers) if l[0] == "bn_add_relu_down"}
        self.below_pw = {i - 1 for i, l in enumerate(layers) if l[0] == PW and i > 0}
        flat = np.asarray(flat, dtype=np.float64)
        assert flat.size == n_logical(in_shape, layers), (flat.size, n_logical(in_shape, layers))
        self.mods, self.kinds, self.outs = [], [], []
        C = in_shape[2]
        sl = iter(tensor_slices(in_shape, layers))
        for l in layers:
            if l[0] in NO_PARAMS:
                self.mods.append(torch.nn.MaxPool2d(2) if l[0] == "pool" else torch.nn.Sequential(torch.nn.AdaptiveAvgPool2d(1), torch.nn.Flatten(1)))
                self.kinds.append(l[0])
                continue
            ws, bs = next(sl)
            if l[0] == PW:
                m = torch.nn.Conv2d(C, l[1], 1).double()
                w = flat[ws].reshape(C, l[1])                                   # W[K = Cin][Cout]
                if w_transposed:
                    assert C == l[1], "the transposed mutant needs a square layer"
                    w = w.T
                w = np.ascontiguousarray(w.T.reshape(l[1], C, 1, 1))
                C = l[1]
            elif l[0] in ("conv", "conv_linear", "conv_linear_s2"):
                m = torch.nn.Conv2d(C, l[1], 3, stride=2 if l[0] == "conv_linear_s2" else 1, padding=1).double()
                w = np.ascontiguousarray(flat[ws].reshape(3, 3, C, l[1]).transpose(3, 2, 0, 1))
                C = l[1]
            elif l[0] in ("bn_relu", "bn_add_relu", "bn_add_relu_down"):
                m = torch.nn.BatchNorm2d(C, eps=eps, momentum=momentum).double()
                w = flat[ws].copy()
            else:
                assert l[0] in ("dense", "dense_relu"), f"unknown layer kind {l[0]!r}"
                k = flat[ws].size // l[1]
                m = torch.nn.Linear(k, l[1]).double()
                w = np.ascontiguousarray(flat[ws].reshape(k, l[1]).T)
            with torch.no_grad():
                m.weight.copy_(torch.from_numpy(w))
                m.bias.copy_(torch.from_numpy(flat[bs].copy()))
            self.mods.append(m)
            self.kinds.append("conv_linear" if l[0] in ("conv_linear_s2", PW) else "bn_relu" if l[0].startswith("bn_add_relu") else l[0])
        self.layers = [(k,) + tuple(l[1:]) if k not in NO_PARAMS else (k,) for k, l in zip(self.kinds, layers)]
        for i, s in self.skips.items():
            assert 0 <= s < i - 1 and self.kinds[i - 1] == "conv_linear", (i, s, self.kinds)
        self.gap_at = self.kinds.index("global_avgpool") if "global_avgpool" in self.kinds else None
        if arithmetic == "float32":
            for m in self.mods:
                m.float()

    def _conv(self, m, t):
        """StrideNet._conv; a 1x1 module rounds its operands under "bf16" whatever its width (it is never the gather-form first layer)"""
        if m.kernel_size != (1, 1):
            return super()._conv(m, t)
        bias = m.bias.detach() if self.drop_bias_grad else m.bias
        if self.operand == "bf16":
            return _rounded_1x1(self.torch)(t, m.weight, bias)
        return self.torch.nn.functional.conv2d(t, m.weight, bias)

    def forward(self, x, train):
        """StrideNet.forward with the two gradient-path mutants"""
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
                src = self.outs[self.skips[i]]
                src = src.detach() if self.drop_skip_share else src
                t = t + (self._shortcut(src, t.shape[1]) if i in self.down else src)
            pre.append(t)
            if kind in ("conv", "bn_relu", "dense_relu"):
                r = torch.relu(t)
                t = r.detach() + t - t.detach() if self.open_gate_below and i in self.below_pw else r
            self.outs.append(t)
        return t


# ---- exact data: a small-integer net whose forward sums are exact in every precision and every summation order ------------------------------
# 4 x 6 x 32 input of integers in -2 .. 2; a 1x1 layer 32 -> 64 with weights in -1 .. 1 and biases in -3 .. 3 (|z| <= 67); batch
# normalisation in evaluation made the identity (exact_case); a second 1x1 layer 64 -> 32 on the ReLU map with two live weights of +-1 per
# output (integers <= 2 * 67 + 3); a global average pool over 24 pixels is not exact, so the head is a dense layer on the flattened
# 4 x 6 x 32 map with weights in -1 .. 1.  Every intermediate is an integer below 2^24 in magnitude and every bf16 operand an integer of at most 8 bits.
X_SPEC = ((4, 6, 32), ((PW, 64), ("bn_relu",), (PW, 32), ("bn_relu",), ("dense", 5)), 3)


def exact_case(seed=0):
    """(parameters, running statistics, x, the integer logits by NumPy int64, the second map) of X_SPEC under evaluation.  The batch
    normalisation layers are made the identity: gamma 1, beta 0, running mean 0 and a running variance with fl32(1 / sqrt(var + eps)) = 1.0f,
    so y = max(0, x) exactly.  The first layer's weights are in -1 .. 1 over 32 inputs in -2 .. 2, so |z| <= 64 + 3."""
    in_shape, layers, B = X_SPEC
    rng = np.random.default_rng(seed)
    H, W, C = in_shape
    x = rng.integers(-2, 3, (B, H, W, C)).astype(np.int64)
    W1, b1 = rng.integers(-1, 2, (C, 64)).astype(np.int64), rng.integers(-3, 4, 64).astype(np.int64)
    W2, b2 = np.zeros((64, 32), dtype=np.int64), rng.integers(-3, 4, 32).astype(np.int64)
    for co in range(32):                                        # two live inputs per output: the second map stays within bf16's 8 bits
        W2[rng.choice(64, 2, replace=False), co] = rng.choice([-1, 1], 2)
    W3, b3 = rng.integers(-1, 2, (H * W * 32, 5)).astype(np.int64), rng.integers(-3, 4, 5).astype(np.int64)
    a1 = np.maximum(0, x.reshape(-1, C) @ W1 + b1)
    assert a1.max() <= 127, "the first map must be exact in bf16"
    a2 = np.maximum(0, a1 @ W2 + b2)
    # the dense head rounds its input to bf16 under "bf16": keep the second map within 8 bits
    assert a2.max() <= 255, a2.max()
    logits = a2.reshape(B, -1) @ W3 + b3
    flat = np.concatenate([W1.ravel(), b1, np.ones(64), np.zeros(64), W2.ravel(), b2, np.ones(32), np.zeros(32), W3.ravel(), b3]).astype(np.float32)
    eps = float(np.float32(1e-5))
    var = np.float32(1.0 - eps)
    assert np.float32(1.0 / np.sqrt(float(var) + eps)) == np.float32(1.0), "fl32(1 / sqrt(var + eps)), the library's invstd, must be 1.0f"
    stats = np.concatenate([np.zeros(64), np.full(64, var), np.zeros(32), np.full(32, var)]).astype(np.float32)
    return flat, stats, x.astype(np.float32), logits, a2


def against_torch(spec, configure, make_optim, micro=1, rtol=4e-4, tag="", ema=0.0):
    """_stride_ref.against_torch for a net with the kind: ONE update of `micro` micro-batches on the device and on the PwNet twin.  ema: the
    decay of an average started before the update; afterwards it is e0 + (1 - decay) (p1 - e0), e0 = the first parameters, of the twin's p1"""
    from _convnet_util import close, dev, make_net, same_bits, step
    in_shape, layers, B = spec
    with layouts():
        flat, data = _twin_checks.update_case(layout_spec(spec), micro)
    net = make_net(spec, "fp32")
    net.set_params(flat)
    configure(net)
    if ema:
        net.set_ema(ema)
    ref = PwNet(in_shape, layers, flat)
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
