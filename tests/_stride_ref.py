"""The float64 torch twin of the two downsampling layer kinds, for tests/test_convnet_stride_plan.py and tests/test_gpu_convnet_stride.py:
("conv_linear_s2", Cout) = Conv2d(Cin, Cout, 3, stride=2, padding=1) and ("bn_add_relu_down", d) = relu(BatchNorm2d(z) + s'), s' the
option-A shortcut F.pad(s[:, :, ::2, ::2], (0, 0, 0, 0, lo, C - Cs - lo)), lo = (C - Cs) / 2, of the output s of the layer d places in front.
`StrideNet` is tests/_torch_ref.py's TorchNet with those two kinds; everything that only needs the flat LAYOUT of a description
(tensor_slices, random_params, close_per_tensor, _twin_checks.compare) takes `layout(layers)`: the same parameter blocks from kinds
_torch_ref knows.  The nets of the GPU file and their data are here, so the CPU file prepares the twin's side from the same cases.
Not a test file: every assert carries its message."""
import numpy as np
from _torch_ref import NO_PARAMS, TorchNet, n_logical, random_params, tensor_slices
from _twin_checks import twin_update, update_case

RTOL = {"fp32": 2e-4, "bf16": 5e-3}        # what one pass makes (the residual tests' bounds)
RTOL_2 = {"fp32": 4e-4, "bf16": 2e-2}      # what a second step has touched
STEPS = 2


def layout(layers):
    """a description with the same parameter blocks and flat layouts, in kinds _torch_ref knows: a strided convolution is a conv_linear
    with a (parameter-free) pool behind it -- the same [W | b] and the same halved map for the dense layer's K -- and a bn_add_relu_down
    layer is a bn_relu"""
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


def block(c):
    """an identity block of width c"""
    return (("conv_linear", c), ("bn_relu",), ("conv_linear", c), ("bn_add_relu", 4))


def down(c):
    """a down block to width c behind a layer of twice the height and width"""
    return (("conv_linear_s2", c), ("bn_relu",), ("conv_linear", c), ("bn_add_relu_down", 4))


# (input shape, layers, batch): the smallest nets at which each thing can go wrong
# A: H != W, M_out = 36 (one partial tile), 2 x 6 output, every parity class has border rows; the source is a ReLU convolution
D_A = ((4, 12, 3), (("conv", 32),) + down(64) + (("global_avgpool",), ("dense", 7)), 3)
# B: M_out = 300 then 75 (full + partial tiles), the last map odd (3 x 5); sources a bn_add_relu and a bn_add_relu_down; Cout 128
D_B = ((12, 20, 3), (("conv_linear", 32), ("bn_relu",)) + block(32) + down(64) + down(128) + (("global_avgpool",), ("dense", 10)), 5)
# C: the source is a pool (no source gate), Cs == C (a plain subsample), a dense layer directly above a self-gated down block
D_C = ((8, 8, 3), (("conv", 32), ("pool",)) + down(32) + (("dense_relu", 32), ("dense", 10)), 2)
# D: M_out = 32768 (256 output tiles: no split-K), the strided layer as layer 0 (no input gradient at all)
D_D = ((32, 32, 32), (("conv_linear_s2", 64), ("bn_relu",), ("global_avgpool",), ("dense", 10)), 128)
NETS = {"a": D_A, "b": D_B, "c": D_C, "d": D_D}
# per net the options of its device run: B's weight gradient in three chunks of 128 pixels, the last partial
OPTIONS = {"a": (), "b": (("pix_per_chunk", 128),), "c": (), "d": ()}


def resnet14(in_shape=(32, 32, 3), B=512):
    """bench_convnet.py's cifar_resnet14: the CIFAR ResNet of 6n + 2 layers, n = 2, at widths 32 / 64 / 128"""
    layers = (("conv_linear", 32), ("bn_relu",)) + block(32) + block(32) + down(64) + block(64) + down(128) + block(128) + (("global_avgpool",), ("dense", 10))
    return (tuple(in_shape), layers, B)


# per net the seeds of its parameters and of its batch.  Chosen from the twin alone; tests/test_convnet_stride_plan.py asserts each property:
# the margin condition of _twin_checks.compare holds in both precisions (test_margin_condition_of_the_comparison_holds), and the
# bf16-operand twin is insensitive to the arithmetic it is run in -- StrideNet(arithmetic="float32") against the float64 one stays within
# 0.3 of the bf16 allowances over the whole schedule (test_bf16_twin_agrees_with_itself_in_float32; the same test shows net b at seeds
# (3, 4) missing its own float64 self by more than an allowance).  A bf16 rounding boundary that the float32 and
# the float64 value of an activation straddle flips one operand by 2^-8 of itself, and batch normalisation over net b's 75 - 1200 rows
# spreads it: at most seeds the twin's OWN two arithmetics differ by more than the allowance there, which measures the reference, not the device.
# Net d: no pre-activation of its 2097152-element bn_relu map lies within float32's reach of zero (the smallest is 2.2e-6; at seed 0 it is
# 8e-9, and the device's ReLU gate -- decided on a float32 value -- differs from the float64 twin's at that one element, which moves the first
# layer's weight gradient by one term of its sum: seven fp32 allowances).
SEEDS = {"a": (0, 1), "b": (6, 7), "c": (0, 1), "d": (24, 25)}


def case(name, seeds=None):
    """(parameters, x, y) of net `name` from its SEEDS (or from `seeds`).  Net d's logits layer carries the biases linspace(-4.5, 4.5): its 128 rows' features are
    means over 256 pixels and barely differ, so by chance some row's two best logits would lie within the comparison's margin bound."""
    in_shape, layers, B = NETS[name]
    seeds = seeds or SEEDS[name]
    flat = random_params(np.random.default_rng(seeds[0]), in_shape, layout(layers))
    if name == "d":
        flat[tensor_slices(in_shape, layout(layers))[-1][1]] = np.linspace(-4.5, 4.5, layers[-1][1]).astype(np.float32)
    rng = np.random.default_rng(seeds[1])
    return flat, rng.standard_normal((B,) + in_shape).astype(np.float32), rng.integers(0, layers[-1][1], B).astype(np.int32)


def _bf16t(t):
    """_torch_ref._bf16 in the tensor's own dtype: round to nearest even to bfloat16, kept as float64 or float32"""
    return t.float().bfloat16().to(t.dtype)


def _rounded_linear(torch):
    """_torch_ref._rounded_op's dense half in the operands' own dtype"""
    class Rounded(torch.autograd.Function):
        @staticmethod
        def forward(ctx, x, w, b):
            xr, wr = _bf16t(x), _bf16t(w)
            ctx.save_for_backward(xr, wr)
            return xr @ wr.T + b

        @staticmethod
        def backward(ctx, g):
            xr, wr = ctx.saved_tensors
            gr = _bf16t(g)
            return gr @ wr, gr.T @ xr, g.sum(0)
    return Rounded.apply


def _rounded_conv(torch):
    """conv2d of any stride (in the operands' own dtype: float64, or float32 for arithmetic = "float32") on operands rounded to bfloat16, forward and backward (_torch_ref._rounded_op with `stride` passed
    to conv2d, conv2d_input and conv2d_weight); other: the padding on the other side (a mutant, below)"""
    F = torch.nn.functional

    class Rounded(torch.autograd.Function):
        @staticmethod
        def forward(ctx, x, w, b, stride, other):
            xr, wr = _bf16t(x), _bf16t(w)
            if other:
                xr = F.pad(xr, (0, 1, 0, 1))
            ctx.save_for_backward(xr, wr)
            ctx.geom = (stride, 0 if other else 1, other)
            return F.conv2d(xr, wr, b, stride=stride, padding=ctx.geom[1])

        @staticmethod
        def backward(ctx, g):
            xr, wr = ctx.saved_tensors
            stride, pad, other = ctx.geom
            gr = _bf16t(g)
            gx = torch.nn.grad.conv2d_input(xr.shape, wr, gr, stride=stride, padding=pad)
            return (gx[:, :, :-1, :-1] if other else gx, torch.nn.grad.conv2d_weight(xr, wr.shape, gr, stride=stride, padding=pad), g.sum((0, 2, 3)), None, None)
    return Rounded.apply


class StrideNet(TorchNet):
    """TorchNet with ("conv_linear_s2", Cout) and ("bn_add_relu_down", d).  self.kinds names a strided convolution "conv_linear" (its
    module has stride 2) and either skip layer "bn_relu", so the flat views are TorchNet's.  self.down: {bn_add_relu_down layer: source}.
    Four options make MUTANTS, never a model of the library: pad_other_side -- the strided convolution reads rows 2 oh + kh and columns
    2 ow + kw (the zero border below and to the right); sample_odd -- the shortcut samples (2h + 1, 2w + 1); lo_zero -- the shortcut's
    channels start at 0; gate_source = False -- TorchNet's dropped source gate on the skip path.
    arithmetic = "float32": the same modules, parameters and operand rounding evaluated in float32 instead of float64 -- what the
    twin makes of the arithmetic the device computes in; used to measure the twin against itself, never as the reference."""

    def __init__(self, in_shape, layers, flat, momentum=0.1, eps=1e-5, operand="f64", gate_source=True, pad_other_side=False, sample_odd=False, lo_zero=False,
                 arithmetic="float64"):
        import torch
        assert arithmetic in ("float64", "float32"), arithmetic
        self.np_dtype = np.float64 if arithmetic == "float64" else np.float32
        self.operand, self.gate_source, self.gate_below = operand, gate_source, True
        self.pad_other_side, self.sample_odd, self.lo_zero = pad_other_side, sample_odd, lo_zero
        self.torch, self.in_shape = torch, tuple(in_shape)
        self.res_layers = [tuple(l) for l in layers]
        self.layers = [("conv_linear", l[1]) if l[0] == "conv_linear_s2" else ("bn_relu",) if l[0] in ("bn_add_relu", "bn_add_relu_down") else tuple(l) for l in layers]
        self.skips = {i: i - l[1] for i, l in enumerate(layers) if l[0] in ("bn_add_relu", "bn_add_relu_down")}
        self.down = {i: i - l[1] for i, l in enumerate(layers) if l[0] == "bn_add_relu_down"}
        flat = np.asarray(flat, dtype=np.float64)
        assert flat.size == n_logical(in_shape, layout(layers)), (flat.size, n_logical(in_shape, layout(layers)))
        self.mods, self.kinds, self.outs = [], [], []
        C = in_shape[2]
        sl = iter(tensor_slices(in_shape, layout(layers)))
        for l in layers:
            if l[0] in NO_PARAMS:
                self.mods.append(torch.nn.MaxPool2d(2) if l[0] == "pool" else torch.nn.Sequential(torch.nn.AdaptiveAvgPool2d(1), torch.nn.Flatten(1)))
                self.kinds.append(l[0])
                continue
            ws, bs = next(sl)
            if l[0] in ("conv", "conv_linear", "conv_linear_s2"):
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
            self.kinds.append("conv_linear" if l[0] == "conv_linear_s2" else "bn_relu" if l[0].startswith("bn_add_relu") else l[0])
        for i, s in self.skips.items():
            assert 0 <= s < i - 1 and self.kinds[i - 1] == "conv_linear", (i, s, self.kinds)
        self.gap_at = self.kinds.index("global_avgpool") if "global_avgpool" in self.kinds else None
        if arithmetic == "float32":
            for m in self.mods:
                m.float()

    def _rounded(self, m, t):
        return _rounded_linear(self.torch)(t, m.weight, m.bias)

    def _conv(self, m, t):
        """a convolution module applied as the library applies it: rounded operands under "bf16" (all but a first layer of 9 Cin <= 32)"""
        F = self.torch.nn.functional
        strided = m.stride == (2, 2)
        other = strided and self.pad_other_side
        if self.operand == "bf16" and 9 * m.in_channels > 32:
            return _rounded_conv(self.torch)(t, m.weight, m.bias, m.stride[0], other)
        return F.conv2d(F.pad(t, (0, 1, 0, 1)), m.weight, m.bias, stride=2) if other else m(t)

    def _shortcut(self, s, C):
        """option A: every second pixel of s, its Cs channels at lo .. lo + Cs - 1 of C"""
        o = 1 if self.sample_odd else 0
        Cs = s.shape[1]
        lo = 0 if self.lo_zero else (C - Cs) // 2
        assert C >= Cs and (C - Cs) % 2 == 0, (C, Cs)
        return self.torch.nn.functional.pad(s[:, :, o::2, o::2], (0, 0, 0, 0, lo, C - Cs - lo))

    def forward(self, x, train):
        """TorchNet.forward with the strided convolution and the shortcut of a bn_add_relu_down layer"""
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
                src = self.outs[s] if self.gate_source else self.outs[s].detach() + pre[s] - pre[s].detach()
                t = t + (self._shortcut(src, t.shape[1]) if i in self.down else src)
            pre.append(t)
            if kind in ("conv", "bn_relu", "dense_relu"):
                t = torch.relu(t)
            self.outs.append(t)
        return t


def against_torch(spec, configure, make_optim, micro=1, rtol=4e-4, tag=""):
    """_twin_checks.against_torch for a net with the new kinds: ONE update of `micro` micro-batches on the device and on the StrideNet twin"""
    from _convnet_util import close, dev, make_net, same_bits, step
    from _torch_ref import close_per_tensor
    in_shape, layers, B = spec
    flat, data = update_case(layout_spec(spec), micro)
    net = make_net(spec, "fp32")
    net.set_params(flat)
    configure(net)
    ref = StrideNet(in_shape, layers, flat)
    lr = twin_update(ref, data, make_optim)
    for x, y in data:
        step(net, dev(net, x), dev(net, y), lr)
    assert not same_bits(net.get_params(), flat), f"{tag}: the update changed nothing"
    worst = close_per_tensor(net.get_params(), ref.params(), in_shape, layout(layers), rtol, f"{tag} parameters")
    worst = max(worst, close(net.get_bn_stats(), ref.bn_stats(), rtol, f"{tag} running statistics"))
    print(f"{tag}: worst share of an allowance = {worst:.3f}")
    net.close()
    return worst
