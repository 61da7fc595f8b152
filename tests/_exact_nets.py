"""Nets whose forward arithmetic is exact, for tests/test_convnet_exact_nets.py (CPU: the proofs) and tests/test_gpu_convnet_exact.py (GPU).
Integer inputs in [-2, 2], weights in {-1, 0, 1} with about `nnz` non-zeros per column, biases in {-2, -1, 0}, the logits layer times a
power of two: every product and every partial sum of every forward GEMM is a small multiple of one power of two, so fp32 sums are exact
in any order, and (where the certificate says so) every operand and every stored map survives rounding to bf16.  On such a net the
device's logits equal the oracle's bit for bit -- and pooling windows tie, pre-activations are exactly 0 and the softmax can be driven
into saturation, none of which Gaussian data does.  Not a test file and not a conftest: every assert carries its message.

exact_net    the net's batch and parameters
certificate  the proof, from the oracle alone, that the forward pass is exact in a precision mode
degeneracy   how many pooling windows tie at a positive maximum, how many pre-activations are exactly 0
walk         the oracle's loss and backward walk restated (as tests/_mix_ref.py does) for a dense target, with the two rules as flags:
             tie = "first" | "last" maximum of a window, gate = ">" | ">=" on the pre-activation.  The defaults are the oracle, bit for
             bit (tests/test_convnet_exact_nets.py); the others are the mutants a test on such a net has to tell from it.  p = starts
             it from given probabilities instead of its own softmax; drop = takes a row, a column, an image, a tap or a pixel out of one
             convolution's backward kernels (DROPS)

The second half makes the BACKWARD pass exact too (the comment above GAP):
exact_backward_net    a net whose softmax is 1 / t on t tied classes and 0 elsewhere to a float32 device, at a power-of-two batch
backward_case         that net for a spec with its f64 reference: gradient, parameters after a plain / momentum / accumulated step, average
backward_certificate  the proof, from the reference alone, that the device owes that reference element for element in a precision mode
coverage, mutants     dZ is alive at the borders, in every image and channel; every mutant changes the reference
BACKWARD_CASES        the cases of part E of the GPU file, with the plan lines of their batches"""
import functools
from collections import namedtuple
from types import SimpleNamespace

import _forms_cases
import numpy as np
from _convnet_util import CIFAR, CONVNET_BF16_NETS, CONVNET_NETS, FUSED_HEAD, HALO_NETS, MNIST, PLAIN_HEAD, POOL_PAIRS

from oracle import convnet_oracle as co

# precision -> (the oracle's keywords, gradient tolerance): the project's tolerances (tests/_oracle_steps.py)
MODES = {"fp32": (dict(operand="f64", stored=False), 2e-4), "bf16": (dict(operand="bf16", stored=False), 5e-3),
         "bf16_stored": (dict(operand="bf16", stored=True), 5e-3)}


def exact_net(spec, seed=0, logit_shift=0, nnz=6):
    """(x, y, ws, bs, flat) of spec = (in_shape, layers, B): x float32 integers in [-2, 2], y int32 labels in [0, classes), ws / bs the f64
    parameters (every one a float32 value), flat their float32 vector in the library's logical layout.  nnz: non-zeros per weight column,
    one number or one per parameter layer; the logits layer is multiplied by 2 ** -logit_shift."""
    in_shape, layers, B = spec
    rng = np.random.default_rng(seed)
    shapes = co.param_shapes(in_shape, layers)
    per_layer = list(nnz) if isinstance(nnz, (tuple, list)) else [nnz] * len(shapes)
    assert len(per_layer) == len(shapes), (per_layer, len(shapes))
    x = rng.integers(-2, 3, (B,) + tuple(in_shape)).astype(np.float32)
    y = rng.integers(0, layers[-1][1], B).astype(np.int32)
    ws, bs = [], []
    for ((k, c), nb), d in zip(shapes, per_layer):
        ws.append(np.where(rng.random((k, c)) < d / k, rng.choice([-1.0, 1.0], (k, c)), 0.0))
        bs.append(rng.integers(-2, 1, nb).astype(np.float64))
    ws[-1] = ws[-1] * 2.0 ** -logit_shift
    bs[-1] = bs[-1] * 2.0 ** -logit_shift
    flat = co.flatten(ws, bs).astype(np.float32)
    assert np.array_equal(flat.astype(np.float64), co.flatten(ws, bs)), "parameters are not float32 values"
    return x, y, ws, bs, flat


def quantum(*arrays):
    """the largest power of two <= 1 of which every entry of every array is an integer multiple"""
    q = 1.0
    for _ in range(64):
        if all(np.array_equal(np.asarray(a) / q, np.rint(np.asarray(a) / q)) for a in arrays):
            return q
        q /= 2.0
    raise AssertionError("the values are not multiples of one power of two above 2**-64")


def certificate(x, ws, bs, layers, mode):
    """Asserts, from the oracle alone, that the forward pass on these values is exact in `mode`: every GEMM's operands are multiples of
    one power-of-two quantum and the sum of the absolute values of its terms, bias included, stays below 2**20 quanta (the fp32
    significand holds 2**24: the margin covers an adder that aligns to the largest term); for the bf16 modes, that the oracle with
    rounded operands (and rounded stored maps) gives the f64 logits.  Returns the largest sum in quanta."""
    assert mode in MODES, mode
    x64 = np.asarray(x, dtype=np.float64)
    quantum(x64, *ws, *bs)
    cache = []
    logits = co.forward(x64, ws, bs, layers, cache)
    worst, pi = 0.0, 0
    for c in cache:
        if c[0] == "pool":
            continue
        a = np.abs(c[1])
        q = quantum(a) * quantum(ws[pi])
        assert np.array_equal(bs[pi] / q, np.rint(bs[pi] / q)), ("a bias is no multiple of its GEMM's quantum", pi)
        worst = max(worst, float((a @ np.abs(ws[pi]) + np.abs(bs[pi])).max() / q))
        pi += 1
    assert worst < 2 ** 20, ("sum of absolute terms in quanta", worst)
    kw = MODES[mode][0]
    if kw["operand"] != "f64":
        assert np.array_equal(co.forward(x64, ws, bs, layers, None, **kw), logits), f"rounding to bf16 changes the logits ({mode})"
    assert np.array_equal(logits.astype(np.float32).astype(np.float64), logits), "the logits are not float32 values"
    return worst


def _forward(x, ws, bs, layers, operand, stored, tie):
    """convnet_oracle.forward, statement for statement, keeping every pre-activation; tie: which maximum of a window the index names"""
    a = np.asarray(x, dtype=np.float64)
    cache, pi = [], 0
    _op = co._op
    for li, l in enumerate(layers):
        if l[0] == "conv":
            N, H, W, C = a.shape
            cols = co._im2col(a)
            op = "f64" if cols.shape[1] <= 32 else operand
            z = _op(cols, op) @ _op(ws[pi], op) + bs[pi]
            y = np.maximum(z, 0).reshape(N, H, W, -1)
            if stored and not (li + 1 < len(layers) and layers[li + 1][0] == "pool"):
                y = co.round_bf16(y)
            cache.append(("conv", cols, y, a.shape, z.reshape(y.shape)))
            a = y; pi += 1
        elif l[0] == "pool":
            N, H, W, C = a.shape
            win = a.reshape(N, H // 2, 2, W // 2, 2, C).transpose(0, 1, 3, 2, 4, 5).reshape(N, H // 2, W // 2, 4, C)
            idx = win.argmax(axis=3) if tie == "first" else 3 - win[:, :, :, ::-1, :].argmax(axis=3)
            p = np.take_along_axis(win, idx[:, :, :, None, :], axis=3)[:, :, :, 0, :]
            if stored:
                p = co.round_bf16(p)
            cache.append(("pool", idx, a.shape, win))
            a = p
        else:
            f = a.reshape(a.shape[0], -1)
            op = "f64" if (li == len(layers) - 1 and co.head_is_fp32(layers)) else operand
            z = _op(f, op) @ _op(ws[pi], op) + bs[pi]
            y = np.maximum(z, 0) if l[0] == "dense_relu" else z
            cache.append((l[0], f, y, a.shape, z))
            a = y; pi += 1
    return a, cache


def degeneracy(x, ws, bs, layers):
    """(pooling windows whose maximum is positive and attained at least twice, [pre-activations equal to 0 per ReLU layer, conv and
    dense_relu, in layer order]) of the f64 forward pass"""
    _, cache = _forward(x, ws, bs, layers, "f64", False, "first")
    ties, zeros = 0, []
    for c in cache:
        if c[0] == "pool":
            win = c[3]
            m = win.max(axis=3, keepdims=True)
            ties += int((((win == m).sum(axis=3) >= 2) & (m[:, :, :, 0, :] > 0)).sum())
        elif c[0] in ("conv", "dense_relu"):
            zeros.append(int((c[4] == 0).sum()))
    return ties, zeros


def one_hot(y, classes):
    T = np.zeros((len(y), classes))
    T[np.arange(len(y)), y] = 1.0
    return T


def logit_gap(logits):
    """the largest spread, over the batch's rows, between a row's largest and smallest logit"""
    z = np.asarray(logits, dtype=np.float64)
    return float((z.max(axis=1) - z.min(axis=1)).max())


# The mutants of a convolution's backward kernels.  "dw-pixel" leaves out the last pixel of the last image AT WHICH dZ IS NOT 0: behind a
# pool the map's corner pixel carries gradient only where it is the first maximum of its window, so on most layers an exact comparison
# (or any other) cannot see the corner itself; the last live pixel is the nearest thing it can see.
# "dx-tap" is the smallest of them: ONE tap of ONE input-gradient element -- tap (0, 0) at the last pixel and input channel of the last image
# at which that tap contributes and the input is positive (where it is 0, the ReLU gate or the pool below discards the element).
DROPS = ("dx-row", "dx-col", "dx-image", "dx-tap", "dw-pixel", "dw-image")


def _note(cert, name, a, b):
    """one backward GEMM a @ b for the certificate: (name, the sum of the absolute values of its terms in quanta of its two operands)"""
    if cert is not None:
        a, b = np.abs(a), np.abs(b)
        cert.append((name, float((a @ b).max()) / (quantum(a) * quantum(b)) if a.size and b.size else 0.0))


def walk(x, T, ws, bs, layers, operand="f64", stored=False, tie="first", gate=">", p=None, drop=None, trace=None, cert=None, forward=None):
    """(loss, logits, gws, gbs) for a dense target T [B, C]: tests/_mix_ref.soft_loss_and_grads, and with a one-hot T the oracle's
    loss_and_grads, restated with the pooling rule and the ReLU gate as flags.  gate ">=" lets the gradient through where the
    pre-activation is exactly 0; tie "last" routes a window's gradient to the last of its equal maxima.
    p [B, C]: the class probabilities the walk starts from INSTEAD of its own softmax (the loss is then taken from the log-softmax of
    the logits, which stays finite where p is 0).  drop = (parameter layer, one of DROPS): that convolution's input gradient without the
    contributions of dZ's last row / last column / last image / of one tap at one pixel and channel, or its weight gradient without dZ's last pixel of the last image /
    without the last image -- the mutants an exact comparison has to tell from the walk.  trace: a list that receives (parameter
    layer, dZ [N, H, W, Cout]) of every convolution; cert: a list that receives _note's record of every backward GEMM and bias sum;
    forward: (*_forward's result for the same values, mode and tie, a dict) where the caller walks them more than once."""
    assert tie in ("first", "last") and gate in (">", ">="), (tie, gate)
    assert drop is None or drop[1] in DROPS, drop
    logits, cache, memo = forward if forward is not None else (*_forward(x, ws, bs, layers, operand, stored, tie), None)

    def opc(a, op):                                                  # _op of an array that every walk over `forward` rounds alike: rounded once
        if memo is None or op == "f64":
            return co._op(a, op)
        if id(a) not in memo:
            memo[id(a)] = (a, co._op(a, op))
        return memo[id(a)][1]
    open_ = (lambda y, z: y > 0) if gate == ">" else (lambda y, z: z >= 0)
    B = logits.shape[0]
    z = logits - logits.max(axis=1, keepdims=True)
    T = np.asarray(T, dtype=np.float64)
    if p is None:
        p = np.exp(z); p /= p.sum(axis=1, keepdims=True)
        with np.errstate(divide="ignore", invalid="ignore"):
            terms = np.where(T != 0, T * np.log(p), 0.0)
    else:
        p = np.asarray(p, dtype=np.float64)
        terms = T * (z - np.log(np.exp(z).sum(axis=1, keepdims=True)))
    loss = float((-terms.sum(axis=1)).mean())
    d = (p - T) / B
    gws, gbs = [None] * len(ws), [None] * len(bs)
    pi = len(ws) - 1
    head32 = co.head_is_fp32(layers)
    _op = co._op
    for bi, (l, c) in enumerate(zip(reversed(layers), reversed(cache))):
        if c[0] == "pool":
            _, idx, shp, _ = c
            N, H, W, C = shp
            g = np.zeros((N, H // 2, W // 2, 4, C))
            np.put_along_axis(g, idx[:, :, :, None, :], d[:, :, :, None, :], axis=3)
            d = g.reshape(N, H // 2, W // 2, 2, 2, C).transpose(0, 1, 3, 2, 4, 5).reshape(N, H, W, C)
        elif c[0] == "conv":
            _, cols, y, shp, pre = c
            N, H, W, C = shp
            dz4 = d * open_(y, pre)
            dz = dz4.reshape(N * H * W, -1)
            if trace is not None:
                trace.append((pi, dz4))
            dzx = dzw = dz
            if drop is not None and drop[0] == pi and drop[1] != "dx-tap":   # ("dx-tap" is taken out of dcols below)
                keep = np.ones((N, H, W, 1))
                if drop[1] == "dw-pixel":                            # (the last pixel of the last image that carries gradient: see DROPS)
                    live = np.flatnonzero((dz4[N - 1] != 0).any(axis=2))
                    keep[N - 1].reshape(H * W)[live[-1:]] = 0.0
                else:
                    keep[{"dx-row": np.s_[:, H - 1], "dx-col": np.s_[:, :, W - 1], "dx-image": np.s_[N - 1], "dw-image": np.s_[N - 1]}[drop[1]]] = 0.0
                if drop[1].startswith("dx"):
                    dzx = (dz4 * keep).reshape(dz.shape)
                else:
                    dzw = (dz4 * keep).reshape(dz.shape)
            small = cols.shape[1] <= 32
            gws[pi] = cols.T @ dzw if small else opc(cols, operand).T @ _op(dzw, operand); gbs[pi] = dz.sum(axis=0)
            dcols = (_op(dzx, operand) @ opc(ws[pi], operand).T).reshape(N, H, W, 9, C)
            _note(cert, (pi, "wgrad"), cols.T, dz); _note(cert, (pi, "bias"), np.ones((1, dz.shape[0])), dz); _note(cert, (pi, "dgrad"), dz, ws[pi].T)
            if drop is not None and drop == (pi, "dx-tap"):           # tap (0, 0) of dZ's pixel (h, w) lands on the input's pixel (h - 1, w - 1)
                a = cols.reshape(N, H, W, 9, C)[N - 1, :-1, :-1, 4, :]    # the input there: at 0 the gate below discards the element, for any test
                live = np.argwhere((dcols[N - 1, 1:, 1:, 0, :] != 0) & (a > 0))
                if len(live):
                    h, w, ci = live[-1]
                    dcols[N - 1, h + 1, w + 1, 0, ci] = 0.0
            dxp = np.zeros((N, H + 2, W + 2, C))
            t = 0
            for kh in range(3):
                for kw in range(3):
                    dxp[:, kh:kh + H, kw:kw + W, :] += dcols[:, :, :, t, :]; t += 1
            if cert is not None:                                     # the nine taps of one input pixel are one sum on the device
                a = np.abs(dcols); ap = np.zeros_like(dxp); t = 0
                for kh in range(3):
                    for kw in range(3):
                        ap[:, kh:kh + H, kw:kw + W, :] += a[:, :, :, t, :]; t += 1
                cert.append(((pi, "dgrad taps"), float(ap.max()) / (quantum(dz) * quantum(ws[pi]))))
            d = dxp[:, 1:-1, 1:-1, :]
            pi -= 1
        else:
            kind, f, y, shp, pre = c
            dz = d * open_(y, pre) if kind == "dense_relu" else d
            op = "f64" if (bi == 0 and head32) else operand
            gws[pi] = opc(f, op).T @ _op(dz, op); gbs[pi] = dz.sum(axis=0)
            d = (_op(dz, op) @ opc(ws[pi], op).T).reshape(shp)
            _note(cert, (pi, "wgrad"), f.T, dz); _note(cert, (pi, "bias"), np.ones((1, dz.shape[0])), dz); _note(cert, (pi, "dgrad"), dz, ws[pi].T)
            pi -= 1
        li = len(layers) - 1 - bi
        if stored and c[0] != "pool" and li > 0 and layers[li - 1][0] in ("conv", "pool"):
            d = co.round_bf16(d)
    return loss, logits, gws, gbs


def worst_move(gws, gbs, ref_gws, ref_gbs):
    """the largest |d| of any one tensor as a fraction of that tensor's scale in the reference (tests/_convnet_util.close's scale)"""
    return max(float(np.abs(a - b).max()) / max(1e-3, float(np.abs(b).max())) for a, b in zip(list(gws) + list(gbs), list(ref_gws) + list(ref_gbs)))


# ---- the cases of tests/test_gpu_convnet_exact.py, proved by tests/test_convnet_exact_nets.py -------------------------------------------------
# (id, net, precision, tiling, options, plan lines, backward too?, max_batch, slots: a value of "halo_f32_slots" or None)
Exact = namedtuple("Exact", "id spec precision tiling options lines backward max_batch slots", defaults=(True, None, None))

DEEP8 = CONVNET_NETS[4]
# Non-zeros per weight column where 6 is too many: the 8-conv net's maps grow past 8 significant bits from its sixth layer on, so its
# deeper layers are thinned -- with these densities it is certified in every mode (at 6 throughout: in fp32 only).
NNZ = {DEEP8[1]: (6, 6, 4, 4, 3, 3, 3, 3, 6)}

# forms cases whose backward pass the GPU file runs too: one (at least) per weight-gradient and input-gradient family.  Left to the
# forward pass alone: the one-chunk twins of the ragged weight-gradient cases and the 1- and 9-chunk twins of the 5-chunk remap cases.
# (bf16-not-pipelined-plain is the ONE case whose input gradient runs on k_conv3x3_halo_bf16, epilogue 3.)
FORMS_BACKWARD = ("fp32-16wide", "fp32-8wide-pairs", "bf16-1cb-reload", "stored-1cb", "stored-pipelined", "wg16-ragged", "wg8-ragged", "wg-first-layer",
                  "wg-stored-ragged", "xcd-remap-fp32-5chunks", "xcd-remap-bf16-5chunks", "bf16-not-pipelined", "bf16-not-pipelined-plain", "bf16-no-lds-tiling",
                  "fp32-implicit-gemm-wgrad", "bf16-implicit-gemm-wgrad", "fp32-unfused-pool-bwd", "fp32-64wide-wgrad", "bf16-64wide-wgrad", "bf16-dense-nk")

# texts some line of a plain case's plan must contain: the kernel families the case is there to hold (tests/_forms_cases.names)
PLAIN_LINES = {
    "convnet-0-fp32": ["k_conv1_fwd_f32<3, 8>", "4x4x32->64 epi 2: k_conv_fwd<3, tile, 64> split-K 2", "k_pool_fwd", "k_head_f32"],
    "convnet-1-fp32": ["k_conv_fwd<3, gather, 32>", "k_pool_fwd", "k_softmax_ce"],
    "convnet-2-fp32": ["k_conv_fwd<3, gather, 64>", "k_pool_fwd", "k_head_f32"],
    "convnet-3-fp32": ["8x8x32->32 epi 4: k_conv3x3_halo_f32<8, 32>"],
    "convnet-4-fp32": ["k_conv1_fwd_f32<3, 16>", "epi 4: k_conv3x3_halo_f32<16, 32>", "split-K 18", "k_pool_fwd"],
    "convnet-bf16-0": ["epi 4: k_conv3x3_halo_bf16p", "k_conv_fwd_bf16<1, tile, 32> split-K 2", "k_head_f32"],
    "convnet-bf16-1": ["epi 4: k_conv3x3_halo_bf16_1cb<32>"],
    "convnet-bf16-2": ["k_conv_fwd_bf16<1, tile, 128> split-K 8", "k_pool_fwd"],
    "convnet-bf16-3": ["epi 4: k_conv3x3_halo_bf16_1cb<32>", "epi 4: k_conv3x3_halo_bf16p", "k_conv_fwd_bf16<3, tile, 128> split-K 9"],
    "halo-0-lds": ["k_conv1_fwd_f32<3, 16>", "epi 4: k_conv3x3_halo_f32<16, 64>"],
    "halo-1-lds": ["k_conv1_fwd_f32<1, 8>", "epi 4: k_conv3x3_halo_f32<8, 32>", "epi 4: k_conv3x3_halo_f32<8, 64>"],
    "halo-2-lds": ["epi 2: k_conv3x3_halo_f32<16, 64>", "epi 4: k_conv3x3_halo_f32<16, 32>", "epi 2: k_conv3x3_halo_f32<8, 32>"],
    "halo-3-lds": ["k_conv1_fwd_f32<3, 8>", "epi 4: k_conv3x3_halo_f32<8, 32>"],
    "halo-4-lds": ["k_conv1_fwd_f32<3, 8>", "k_head_f32, 2 workgroups"],
    "halo-5-lds": ["k_conv1_fwd_f32<1, 16>", "epi 4: k_conv3x3_halo_f32<8, 32>"],
    "pool-pairs-fp32": ["epi 4: k_conv3x3_halo_f32<8, 64>", "k_head_f32, 2 workgroups"],
    "pool-pairs-stored": ["epi 4: k_conv3x3_halo_bf16p", "bf16 input map"],
    "halo-0-bf16": ["epi 4: k_conv3x3_halo_bf16p"], "halo-1-bf16": ["epi 4: k_conv3x3_halo_bf16_1cb<32>", "epi 4: k_conv3x3_halo_bf16p"],
    "halo-2-bf16": ["epi 4: k_conv3x3_halo_bf16p", "k_conv_fwd_bf16<3, tile, 64> split-K 2"], "halo-3-bf16": ["epi 4: k_conv3x3_halo_bf16p"],
    "halo-5-bf16": ["epi 4: k_conv3x3_halo_bf16p"], "halo-0-stored": ["epi 4: k_conv3x3_halo_bf16p", "bf16 input map"], "halo-4-stored": ["bf16 input map"],
}

# Nets the library accepts under bf16 storage and the tiling at which it does (None: "auto"; "lds" for the nets of the halo file, whose
# tiling it is, and for nets it accepts at no other).  A net that is not here is refused at "auto" and at "lds": its convolutions do not
# all run on the LDS-tiled kernels with fused pooling.  tests/test_convnet_exact_nets.py holds this table against the plan.
STORED_TILING = {CONVNET_NETS[2]: "lds", CONVNET_BF16_NETS[2]: "lds", HALO_NETS[0]: "lds", HALO_NETS[4]: "lds", POOL_PAIRS: None, _forms_cases.PAIRS8: None,
                 _forms_cases.STORED: None, _forms_cases.WG8: None, _forms_cases.WG_FIRST: None, _forms_cases.WG_STORED: None, _forms_cases.BF16_HALO: None,
                 _forms_cases.WIDTHS64: None, _forms_cases._flat48(4): "lds", _forms_cases._flat48(20): "lds", _forms_cases._flat48(36): "lds",
                 _forms_cases.DENSE_NK: "lds"}


def plain_nets():
    """(name, net, tiling) of every net of the GPU file: the nets of tests/test_gpu_convnet.py, of tests/test_gpu_convnet_halo.py (tiling
    "lds"), POOL_PAIRS, and every net of tests/_forms_cases.py once, without its cases' options"""
    nets = [(f"convnet-{i}", s, None) for i, s in enumerate(CONVNET_NETS)] + [("convnet-wide130", CONVNET_BF16_NETS[2], None)]
    nets += [(f"halo-{i}", s, "lds") for i, s in enumerate(HALO_NETS)] + [("pool-pairs", POOL_PAIRS, None)]
    seen = {s for _, s, _ in nets}
    for c in _forms_cases.CASES:
        if c.spec not in seen:
            seen.add(c.spec)
            nets.append(("net-of-" + c.id, c.spec, None))
    return nets


def gpu_cases():
    """Every case of the GPU file: the nets of tests/test_gpu_convnet.py in fp32 and (its bf16 test's four) in bf16, the nets of
    tests/test_gpu_convnet_halo.py in fp32 with tiling "lds", POOL_PAIRS in fp32 and bf16 storage, every forms case in its own precision
    with its own options -- these forward and backward (the forms cases thinned to FORMS_BACKWARD) -- and then, forward only, every net
    of plain_nets() in bf16 and, where the library accepts it (STORED_TILING), under bf16 storage, unless a case above has that pair."""
    cases = [Exact(f"convnet-{i}-fp32", s, "fp32", None, {}, []) for i, s in enumerate(CONVNET_NETS)]
    cases += [Exact(f"convnet-bf16-{i}", s, "bf16", None, {}, []) for i, s in enumerate(CONVNET_BF16_NETS)]
    cases += [Exact(f"halo-{i}-lds", s, "fp32", "lds", {}, []) for i, s in enumerate(HALO_NETS)]
    cases += [Exact("pool-pairs-fp32", POOL_PAIRS, "fp32", None, {}, []), Exact("pool-pairs-stored", POOL_PAIRS, "bf16_stored", None, {}, [])]
    cases += [Exact("forms-" + c.id, c.spec, c.precision, c.tiling, c.options, c.lines, c.id in FORMS_BACKWARD) for c in _forms_cases.CASES]
    cases += [Exact("forms-" + c.id + "-2slots", c.spec, c.precision, c.tiling, c.options, c.lines, False, None, 2) for c in _forms_cases.LOOPS]
    cases += [Exact("fused-head-max-batch-16", FUSED_HEAD, "fp32", None, {}, [], True, 16)]
    have = {(c.spec, c.precision) for c in cases}
    for name, spec, tiling in plain_nets():
        if (spec, "bf16") not in have:
            cases.append(Exact(name + "-bf16", spec, "bf16", tiling, {}, [], False))
        if spec in STORED_TILING and (spec, "bf16_stored") not in have:
            cases.append(Exact(name + "-stored", spec, "bf16_stored", STORED_TILING[spec], {}, [], False))
    return [c._replace(lines=PLAIN_LINES[c.id]) if c.id in PLAIN_LINES else c for c in cases]


def _shift_into(gap, lo, hi):
    """the logit_shift of smallest magnitude that brings a raw logit gap into [lo, hi] (hi >= 2 * lo, or lo == 0)"""
    if gap > hi:
        return int(np.ceil(np.log2(gap / hi)))
    if gap < lo:
        return -int(np.ceil(np.log2(lo / gap)))
    return 0


@functools.lru_cache(maxsize=None)
def exact_case(spec, kind="gradient", seed=0):
    """exact_net(spec, seed) with its logit_shift chosen from the oracle's raw logits: kind "gradient" -- the gap is at most 16, so the
    softmax is alive and every layer's gradient carries weight; kind "saturated" -- the gap lies in [120, 600], where expf underflows.
    A namespace of x, y, ws, bs, flat, shift, logits (f64) and gap; the arrays are read-only and shared."""
    in_shape, layers, _ = spec
    nnz = NNZ.get(layers, 6)
    x, y, ws, bs, _ = exact_net(spec, seed, 0, nnz)
    raw = logit_gap(co.forward(x.astype(np.float64), ws, bs, layers))
    shift = _shift_into(raw, 0, 16) if kind == "gradient" else _shift_into(raw, 120, 600)
    x, y, ws, bs, flat = exact_net(spec, seed, shift, nnz)
    logits = co.forward(x.astype(np.float64), ws, bs, layers)
    case = SimpleNamespace(spec=spec, x=x, y=y, ws=tuple(ws), bs=tuple(bs), flat=flat, shift=shift, logits=logits, gap=logit_gap(logits))
    for a in [x, y, flat, logits, *ws, *bs]:
        a.setflags(write=False)
    return case


EVAL_ROWS = {FUSED_HEAD: 13, PLAIN_HEAD: 8, POOL_PAIRS: 150}          # no multiple of the net's max_batch (5, 3, 64)


def eval_set(spec):
    """a uint8 set of EVAL_ROWS[spec] rows with pixels 0 .. 4 -- under x_scale 1, x_shift -2 the integers -2 .. 2 -- and its labels"""
    in_shape, layers, _ = spec
    rows = EVAL_ROWS[spec]
    rng = np.random.default_rng(rows)
    return rng.integers(0, 5, (rows,) + tuple(in_shape)).astype(np.uint8), rng.integers(0, layers[-1][1], rows).astype(np.int32)


@functools.lru_cache(maxsize=None)
def reference(spec, precision, lr, backward=True):
    """The gradient case of `spec` with what tests/_oracle_steps.check_oracle reads: the oracle's logits, and (backward) its loss,
    gradient and two SGD steps at rate lr in `precision`'s mode.  The logits are the f64 ones: the certificate says the mode's are equal."""
    case = exact_case(spec)
    in_shape, layers, _ = spec
    ref = SimpleNamespace(**vars(case))
    if backward:
        kw = {k: v for k, v in MODES[precision][0].items() if k != "operand" or v != "f64"}
        x64, ws, bs = case.x.astype(np.float64), list(case.ws), list(case.bs)
        ref.loss, logits, gws, gbs = co.loss_and_grads(x64, case.y, ws, bs, layers, **kw)
        assert np.array_equal(logits, case.logits), "the mode's logits are not the f64 logits: the certificate does not hold"
        w1, b1 = [w - lr * g for w, g in zip(ws, gws)], [b - lr * g for b, g in zip(bs, gbs)]      # (convnet_oracle.sgd_step's statement)
        w2, b2, ref.loss1 = co.sgd_step(x64, case.y, w1, b1, layers, lr, **kw)
        ref.grad, ref.params1, ref.params2 = co.flatten(gws, gbs), co.flatten(w1, b1), co.flatten(w2, b2)
        for a in (ref.grad, ref.params1, ref.params2):
            a.setflags(write=False)
    return ref


# ---- the backward pass made exact too ---------------------------------------------------------------------------------------------------------
# The softmax is the one inexact quantity at the top of the backward walk.  Here the first t columns of the logits layer are identical (t a
# power of two: those classes tie at the maximum of every sample) and every other class has its bias lowered by a power of two until it
# sits at least 120 below them, where expf underflows: exp(z - max) is 1 on the tied classes and 0 elsewhere, p = 1 / t, and with a
# power-of-two batch d = (p - T) / B is a multiple of 1 / (t B).  Below that every operand is a small multiple of a power of two, so every
# sum of the backward walk is exact in fp32 in any order and survives bf16 rounding: the device's gradient must EQUAL the f64 reference's.
GAP = 120.0                                              # expf(-120) is 0 in float32 (the smallest subnormal is exp(-103.3))
STEP_LR = 2.0 ** -3                                      # the rate of every step on these nets
SGD = (0.5, 2.0 ** -4, True)                             # set_sgd(momentum, weight decay, nesterov) of the "sgd" cases
EMA, ACCUM = 0.5, 2                                      # set_ema's decay, set_accumulate's k (accum_c = 0.5)
SMOOTH, PAIR_W = 0.125, 0.25                             # the soft cases: eps / C = 2 ** -6 on 8 classes; the pair step's weight
BACKWARD_NNZ = {"conv": 3.5, "dense_relu": 20, "dense": None}      # non-zeros per column by layer kind; the logits layer is dense


def tied_classes(classes):
    """t: 4, or where the net has fewer than 5 classes the largest power of two that leaves one class to push down"""
    t = 4
    while t >= classes:
        t //= 2
    assert t >= 1, classes
    return t


def exact_backward_net(spec, seed=0, nnz=None, batches=1):
    """(x, y, ws, bs, flat, push, t) of spec = (in_shape, layers, B), B a power of two: x float32 in {-1, 0, 1} ([batches * B, ...]: that
    many batches of B rows, one after the other), weights in {-1, 0, 1} with about nnz non-zeros per column (one number per parameter
    layer; None: BACKWARD_NNZ by layer kind), biases in {0, 1, 2}, a dense +-1 logits layer whose first t columns are one column, the other
    classes' biases lowered by `push` (a power of two) so that on every row each sits at least GAP below the tied ones, and int32 labels
    y drawn from the lowered classes."""
    in_shape, layers, B = spec
    assert B >= 1 and B & (B - 1) == 0, ("the batch is no power of two", B)
    rng = np.random.default_rng(seed)
    shapes = co.param_shapes(in_shape, layers)
    kinds = [l[0] for l in layers if l[0] != "pool"]
    per_layer = list(nnz) if nnz is not None else [BACKWARD_NNZ[k] for k in kinds]
    assert len(per_layer) == len(shapes), (per_layer, len(shapes))
    classes = layers[-1][1]
    t = tied_classes(classes)
    x = rng.integers(-1, 2, (batches * B,) + tuple(in_shape)).astype(np.float32)
    ws, bs = [], []
    for ((k, c), nb), d in zip(shapes[:-1], per_layer):
        ws.append(np.where(rng.random((k, c)) < d / k, rng.choice([-1.0, 1.0], (k, c)), 0.0))
        bs.append(rng.integers(0, 3, nb).astype(np.float64))
    (k, c), nb = shapes[-1]
    w, b = rng.choice([-1.0, 1.0], (k, c)), rng.integers(0, 3, nb).astype(np.float64)
    w[:, :t] = w[:, :1]; b[:t] = b[0]
    raw = co.forward(x.astype(np.float64), ws + [w], bs + [b], layers)
    assert (raw[:, :t] == raw[:, :1]).all(), "the tied classes do not tie"
    excess = float((raw[:, t:].max(axis=1) - raw[:, 0]).max()) + GAP
    push = 2.0 ** max(0, int(np.ceil(np.log2(max(excess, 1.0)))))
    b[t:] -= push
    ws.append(w); bs.append(b)
    y = (t + rng.integers(0, classes - t, batches * B)).astype(np.int32)
    flat = co.flatten(ws, bs).astype(np.float32)
    assert np.array_equal(flat.astype(np.float64), co.flatten(ws, bs)), "parameters are not float32 values"
    return x, y, ws, bs, flat, push, t


def limit_softmax(B, classes, t):
    """what the softmax of such logits is to a float32 device: 1 / t on the tied classes, 0 elsewhere"""
    p = np.zeros((B, classes))
    p[:, :t] = 1.0 / t
    return p


def is_f32(a):
    a = np.asarray(a, dtype=np.float64)
    with np.errstate(over="ignore"):
        return bool(np.array_equal(a.astype(np.float32).astype(np.float64), a))


# (id, net, precision, tiling, options, plan lines, slots, extra: None | "sgd" | "ema" | "accum" | "soft")
Back = namedtuple("Back", "id spec precision tiling options lines slots extra", defaults=((), None, None))


@functools.lru_cache(maxsize=None)
def backward_case(spec, extra=None, seed=0):
    """The exact-backward net of `spec` with its reference, everything in f64 and from the restated walk started at the limit softmax:
    x, y, ws, bs, flat, push, t, T (the dense target), p, logits, loss, gws, gbs, grad (flat), params1 (after one plain step at STEP_LR);
    extra "sgd": sgd_params, sgd_velocity after one step under set_sgd(*SGD); "ema": ema after one plain step under set_ema(EMA);
    "accum": a second batch x2, y2 with T2, grad2, acc1 (the accumulator after the first micro-step) and accum_params (after the second);
    "soft": T is the target smoothed by SMOOTH, and yb, pair_T, pair_loss, pair_params are a pair step at weight PAIR_W under it.
    Arrays are read-only and shared."""
    from _sgd_ref import sgd_update
    in_shape, layers, B = spec
    classes = layers[-1][1]
    x, y, ws, bs, flat, push, t = exact_backward_net(spec, seed, BACKWARD_NNZ_OF.get(layers), 2 if extra == "accum" else 1)
    c = SimpleNamespace(spec=spec, extra=extra, x=x[:B], y=y[:B], ws=tuple(ws), bs=tuple(bs), flat=flat, push=push, t=t, p=limit_softmax(B, classes, t))
    x64 = c.x.astype(np.float64)
    eps = SMOOTH if extra == "soft" else 0.0
    c.T = soft_targets(c.y, c.y, 1.0, eps, classes)
    c.loss, c.logits, gws, gbs = walk(x64, c.T, ws, bs, layers, p=c.p)
    c.gws, c.gbs, c.grad = tuple(gws), tuple(gbs), co.flatten(gws, gbs)
    flat64 = co.flatten(ws, bs)
    c.params1 = flat64 - STEP_LR * c.grad
    if extra == "sgd":
        c.sgd_params, c.sgd_velocity = sgd_update(flat64, c.grad, np.zeros_like(flat64), STEP_LR, *SGD)
    elif extra == "ema":
        c.ema = flat64 + (1.0 - EMA) * (c.params1 - flat64)
    elif extra == "accum":
        c.x2, c.y2 = x[B:], y[B:]
        c.T2 = one_hot(c.y2, classes)
        _, c.logits2, g2w, g2b = walk(c.x2.astype(np.float64), c.T2, ws, bs, layers, p=c.p)
        c.grad2 = co.flatten(g2w, g2b)
        c.acc1 = c.grad / ACCUM
        c.accum_params = flat64 - STEP_LR * (c.acc1 + c.grad2 / ACCUM)
    elif extra == "soft":
        c.yb = (t + np.random.default_rng(seed + 7).integers(0, classes - t, B)).astype(np.int32)
        c.pair_T = soft_targets(c.y, c.yb, PAIR_W, eps, classes)
        c.pair_loss, _, pw, pb = walk(x64, c.pair_T, ws, bs, layers, p=c.p)
        c.pair_grad = co.flatten(pw, pb)
        c.pair_params = flat64 - STEP_LR * c.pair_grad
    for a in vars(c).values():
        if isinstance(a, np.ndarray):
            a.setflags(write=False)
    for a in [*ws, *bs, *gws, *gbs]:
        a.setflags(write=False)
    return c


def soft_targets(ya, yb, w, eps, C):
    """tests/_mix_ref.soft_targets (not imported: that module pulls in the recipe restatements)"""
    ya, yb = np.asarray(ya), np.asarray(yb)
    return (1.0 - eps) * (w * one_hot(ya, C) + (1.0 - w) * one_hot(yb, C)) + eps / C


def backward_certificate(c, mode):
    """Asserts, from the reference alone, that the backward pass of backward_case `c` is exact in `mode` and that the limit softmax is
    the right reference for a float32 device:
      the forward certificate (so the logits are the f64 ones in the mode);
      the f64 softmax of the logits differs from the limit by less than 2 ** -149, the smallest float32, in every entry;
      every backward GEMM (dZ . W^T with the nine taps of a pixel as one sum, cols^T . dZ, the bias sums, the dense layers) has operands on
      one quantum and a sum of absolute terms below 2 ** 20 quanta -- the forward certificate's rule and margin;
      the walk in `mode` gives the f64 gradient, element for element;
      the gradient, the parameters after one update and the case's velocity / average / accumulator are float32 values.
    Returns the largest backward sum in quanta."""
    in_shape, layers, B = c.spec
    kw = MODES[mode][0]
    ws, bs = list(c.ws), list(c.bs)
    batches = [(c.x, c.T, c.logits, (c.gws, c.gbs))] + ([(c.x2, c.T2, c.logits2, None)] if c.extra == "accum" else [])
    worst = 0.0
    for x, T, logits, grads in batches:
        x64 = x.astype(np.float64)
        certificate(x, ws, bs, layers, mode)
        z = logits - logits.max(axis=1, keepdims=True)
        soft = np.exp(z) / np.exp(z).sum(axis=1, keepdims=True)
        assert float(np.abs(soft - c.p).max()) < 2.0 ** -149, ("the f64 softmax is not the limit to a float32", float(np.abs(soft - c.p).max()))
        assert (np.exp(z.astype(np.float32)) == (z == 0)).all(), "float32 exp is not 1 on the tied classes and 0 elsewhere"
        cert = []
        _, _, gws, gbs = walk(x64, T, ws, bs, layers, p=c.p, cert=cert)
        worst = max([worst] + [s for _, s in cert])
        assert worst < 2 ** 20, ("sum of absolute terms in quanta", max(cert, key=lambda r: r[1]))
        if kw["operand"] != "f64":
            _, m_logits, m_gws, m_gbs = walk(x64, T, ws, bs, layers, p=c.p, **kw)
            assert np.array_equal(m_logits, logits), f"rounding to bf16 changes the logits ({mode})"
            for k, (a, b) in enumerate(zip(m_gws + m_gbs, gws + gbs)):
                assert np.array_equal(a, b), f"rounding to bf16 changes gradient tensor {k} ({mode})"
        if grads is not None:
            assert all(np.array_equal(a, b) for a, b in zip(gws + gbs, list(grads[0]) + list(grads[1]))), "the reference is not the walk's gradient"
    names = ["grad", "params1"] + {"sgd": ["sgd_params", "sgd_velocity"], "ema": ["ema"], "accum": ["grad2", "acc1", "accum_params"],
                                   "soft": ["pair_grad", "pair_params"]}.get(c.extra, [])
    for name in names:
        assert is_f32(getattr(c, name)), f"{name} is not an array of float32 values"
    return worst


COVERAGE = dict(pixels=0.45, border=0.20, channels=0.45)  # the least shares of dZ != 0 per convolution layer (conditions, not measurements)


def coverage(c):
    """Per convolution layer (parameter layer, shares): dZ != 0 at which share of the pixels, of the pixels of each of the map's four
    borders over the batch (the least of the four), of the images, of the channels.  Asserts COVERAGE and every image."""
    in_shape, layers, B = c.spec
    trace = []
    walk(c.x.astype(np.float64), c.T, list(c.ws), list(c.bs), layers, p=c.p, trace=trace)
    out = []
    for pi, dz in trace:
        live = (dz != 0).any(axis=3)                                 # [N, H, W]: some channel of the pixel
        borders = min(float(live[:, 0].mean()), float(live[:, -1].mean()), float(live[:, :, 0].mean()), float(live[:, :, -1].mean()))
        shares = dict(pixels=float(live.mean()), border=borders, images=float(live.any(axis=(1, 2)).mean()), channels=float((dz != 0).any(axis=(0, 1, 2)).mean()))
        assert shares["pixels"] >= COVERAGE["pixels"] and shares["border"] >= COVERAGE["border"] and shares["images"] == 1.0 \
            and shares["channels"] >= COVERAGE["channels"], ("dZ is not alive enough in parameter layer", pi, shares)
        out.append((pi, shares))
    return out


def mutants(c, mode="fp32"):
    """[(flags of walk, tensors of the gradient that differ from the reference's)] of every mutant that applies to the case: the last
    maximum (nets with a pool), the gate at zero, and per convolution layer the five DROPS (the input-gradient ones where a parameter
    layer lies in front of the convolution).  The comparison is exact: one differing tensor is a detection."""
    in_shape, layers, B = c.spec
    kw = MODES[mode][0]
    x64, ws, bs = c.x.astype(np.float64), list(c.ws), list(c.bs)
    flags = [dict(gate=">=")] + ([dict(tie="last")] if any(l[0] == "pool" for l in layers) else [])
    pi = 0
    for l in layers:
        if l[0] == "conv":
            flags += [dict(drop=(pi, what)) for what in DROPS if pi > 0 or what.startswith("dw")]
        pi += l[0] != "pool"
    ref = list(c.gws) + list(c.gbs)
    out = []
    first = (*_forward(x64, ws, bs, layers, kw["operand"], kw["stored"], "first"), {})
    for f in flags:
        _, _, gws, gbs = walk(x64, c.T, ws, bs, layers, p=c.p, **kw, **f, forward=None if "tie" in f else first)
        out.append((f, [k for k, (a, b) in enumerate(zip(gws + gbs, ref)) if not np.array_equal(a, b)]))
    return out


def at(spec, B):
    return (spec[0], spec[1], B)


# the soft cases' net: 8 classes (SMOOTH / 8 = 2 ** -6), a head the library fuses (k_head_f32) unless "head" is 0 (k_softmax_ce_soft)
SOFT8 = ((8, 8, 3), (("conv", 32), ("pool",), ("conv", 64), ("pool",), ("dense_relu", 32), ("dense", 8)), 4)
# non-zeros per column where BACKWARD_NNZ is too many or too few for a net (keyed by its layers)
BACKWARD_NNZ_OF = {}

_F = _forms_cases
_W4, _P8, _S8 = at(_F.WIDE16, 4), at(_F.PAIRS8, 8), at(_F.STORED, 8)
# BF16_HALO_PLAIN: below 22 images its 3 x 3 layers have fewer than 256 output tiles and split K on the implicit-GEMM kernels; 32 is the
# smallest power of two at which they run on the LDS-tiled bf16 kernels with epilogues 2 and 3 (what its forms cases are there for).  16 is kept
# as a case of its own: the split-K input gradients with epilogue 3.
_PL16, _PL32 = at(_F.BF16_HALO_PLAIN, 16), at(_F.BF16_HALO_PLAIN, 32)
# The first layer's weight gradient aims at 1024 workgroups, 128 chunks of its 8 tiles.  WG_FIRST's 24 x 16 map has 3 pixel blocks per image:
# at a power-of-two batch its chunks come out even (64 images: 96 chunks of 2).  A 40 x 16 map has 5: 320 blocks in 107 chunks of 3, the last of 2.
_WG_FIRST40 = ((40, 16, 3), _F.WG_FIRST[1], 64)
_REMAP16 = {"xcd_remap": 1, "pix_per_chunk": 128}
_REMAP16H = dict(_REMAP16, halo_wgrad=0)


# texts some line of the case's plan must contain (tests/_forms_cases.names): the backward kernel forms the case is there for, with the item
# and chunk counts of ITS batch
_W4_LINES = ["8x16x96->96 epi 0 pooled-in: k_conv3x3_halo_f32<16, 32>, 12 items", "16x32x96->32 epi 3 pooled-in: k_conv3x3_halo_f32<16, 32>, 16 items",
             "8x16x96->96 pooled-dZ: k_wgrad3x3_halo_f32<16>, 4 chunks x 9 tiles", "16x32x32->96 pooled-dZ: k_wgrad3x3_halo_f32<16>, 16 chunks x 3 tiles",
             "16x32x3->32: k_conv1_wgrad_f32<3, 16>, 16 chunks", "k_reduce_all"]
_P8_LINES = ["12x12x64->64 epi 0 pooled-in: k_conv3x3_halo_f32<16, 64>, 16 items", "24x24x64->32 epi 3 pooled-in: k_conv3x3_halo_f32<8, 32>, 36 items",
             "24x24x32->64 pooled-dZ: k_wgrad3x3_halo_f32<8>, 36 chunks x 2 tiles", "24x24x1->32: k_conv1_wgrad_f32<1, 8>, 36 chunks"]
_W4_BF16_LINES = ["16x32x32->96 epi 4: k_conv3x3_halo_bf16_1cb<32>, 48 items", "16x32x96->32 epi 3: k_conv_fwd_bf16<3, tile, 32> split-K 6", "k_pool_bwd",
                  "16x32x32->96: k_wgrad3x3_halo_bf16<32, 32>, 2 chunks x 3 tiles", "8x16x96->96: k_conv_wgrad_bf16<3, 32, 3>, 2 chunks"]
_S8_LINES = ["12x16x64->64 epi 3 pooled-in: k_conv3x3_halo_bf16p, 16 items", "12x16x64->32 epi 0: k_conv3x3_halo_bf16p, 16 items",
             "12x16x64->64 pooled-dZ: k_wgrad3x3_halo_bf16<64, 64>, 2 chunks x 1 tiles", "24x32x32->32 pooled-dZ: k_wgrad3x3_halo_bf16<32, 32>, 6 chunks x 1 tiles",
             "24x32x1->32: k_conv1_wgrad_f32<1, 16>, 48 chunks", "bf16 output map"]
_PL32_LINES = ["16x32x96->32 epi 3: k_conv_fwd_bf16<3, tile, 32> split-K 4", "16x32x32->96: k_wgrad3x3_halo_bf16<32, 32>, 16 chunks x 3 tiles",
               "16x32x96->64: k_conv_wgrad_bf16<3, 32, 3>, 32 chunks", "k_pool_bwd"]
_LOOP_LINES = {
    "fp32-16wide": _W4_LINES, "fp32-8wide-pairs": _P8_LINES, "bf16-1cb-reload": _W4_BF16_LINES,
    "stored-1cb": _S8_LINES + ["24x32x32->32 epi 3 pooled-in: k_conv3x3_halo_bf16_1cb<32>, 48 items"],
    "stored-pipelined": _S8_LINES + ["24x32x32->32 epi 3 pooled-in: k_conv3x3_halo_bf16p, 48 items"],
    "bf16-pipelined-3-column-blocks": _PL32_LINES + ["16x32x32->96 epi 2: k_conv3x3_halo_bf16_1cb<32>, 384 items", "16x32x64->96 epi 3: k_conv3x3_halo_bf16p, 384 items"],
}
BACKWARD_LINES = dict(_LOOP_LINES)
BACKWARD_LINES.update({f"{k}-{s}slots": v for k, v in _LOOP_LINES.items() for s in (2, 3)})
BACKWARD_LINES.update({
    # 16 pixel blocks in chunks of 3 (the last of 1) and of 6 (the last of 4); 18 in chunks of 5 (the last of 3)
    "wg16-ragged": ["16x32x32->32: k_wgrad3x3_halo_f32<16>, 6 chunks x 1 tiles", "16x32x32->96 pooled-dZ: k_wgrad3x3_halo_f32<16>, 3 chunks x 3 tiles"],
    "wg8-ragged": ["24x24x32->32: k_wgrad3x3_halo_f32<8>, 6 chunks x 1 tiles", "24x24x32->64 pooled-dZ: k_wgrad3x3_halo_f32<8>, 4 chunks x 2 tiles"],
    # 192 pixel blocks in 96 chunks of 2; 320 in 107 chunks of 3, the last of 2
    "wg-first-layer": ["24x16x3->256 pooled-dZ: k_conv1_wgrad_f32<3, 16>, 96 chunks"],
    "wg-first-layer-ragged": ["40x16x3->256 pooled-dZ: k_conv1_wgrad_f32<3, 16>, 107 chunks"],
    # bf16 storage: 16 pixel blocks in 2 chunks of 8 (the kernel's least chunk: no power-of-two batch leaves this net a shorter one)
    "wg-stored-2-chunks": ["16x32x32->32 pooled-dZ: k_wgrad3x3_halo_bf16<32, 32>, 2 chunks x 1 tiles", "16x32x32->32 epi 3 pooled-in: k_conv3x3_halo_bf16_1cb<32>, 16 items",
                         "8x16x64->32 epi 0: k_conv3x3_halo_bf16p, 4 items"],
    "bf16-not-pipelined": ["16x16x32->64 epi 4: k_conv3x3_halo_bf16", "8x8x64->32 epi 4: k_conv3x3_halo_bf16", "8x8x64->32: k_wgrad3x3_halo_bf16<64, 32>, 1 chunks x 1 tiles"],
    "bf16-not-pipelined-plain": _PL32_LINES + ["16x32x32->96 epi 2: k_conv3x3_halo_bf16", "16x32x64->96 epi 3: k_conv3x3_halo_bf16"],
    "bf16-plain-b16-split-k": ["16x32x64->96 epi 3: k_conv_fwd_bf16<3, tile, 32> split-K 2", "16x32x32->96: k_wgrad3x3_halo_bf16<32, 32>, 8 chunks x 3 tiles"],
    "bf16-no-lds-tiling": ["16x16x32->64 epi 2: k_conv_fwd_bf16<3, tile,", "8x8x32->64 epi 3: k_conv_fwd_bf16<3, tile, 64> split-K 2", "k_pool_fwd", "k_pool_bwd"],
    "bf16-implicit-gemm-wgrad": ["16x16x32->64: k_conv_wgrad_bf16<3, 32, 3>, 4 chunks", "8x8x64->32: k_conv_wgrad_bf16<3, 32, 3>, 1 chunks", "k_pool_bwd"],
    "fp32-implicit-gemm-wgrad": ["epi 3: k_conv3x3_halo_f32<16, 32>, 16 items", "k_pool_bwd", "16x32x3->32: k_conv_wgrad<3, gather, 32>, 2 chunks",
                                 "16x32x32->96: k_conv_wgrad<3, tile, 32>, 2 chunks", "8x16x96->96: k_conv_wgrad<3, tile, 32>, 1 chunks"],
    "fp32-unfused-pool-bwd": ["k_pool_bwd", "8x16x96->96 epi 0: k_conv3x3_halo_f32<16, 32>, 12 items", "16x32x96->32 epi 3: k_conv3x3_halo_f32<16, 32>, 16 items",
                              "16x32x32->96: k_wgrad3x3_halo_f32<16>, 16 chunks x 3 tiles", "8x16x96->96: k_wgrad3x3_halo_f32<16>, 4 chunks x 9 tiles"],
    "fp32-64wide-wgrad": ["8x8x64->64: k_conv_wgrad<3, tile, 64>", "1x1x1024->64: k_conv_wgrad<1, tile, 64>"],
    "bf16-64wide-wgrad": ["8x8x64->64: k_conv_wgrad_bf16<3, 64, 3>", "1x1x1024->64: k_conv_wgrad_bf16<1, 64, 4>"],
    "fp32-dense-nk": ["1x1x128->64: k_conv_wgrad<1, tile, 32>", "k_softmax_ce"],
    "bf16-dense-nk": ["1x1x128->64: k_conv_wgrad_bf16<1, 32, 4>", "1x1x64->32: k_conv_wgrad_bf16<1, 32, 2>", "1x1x32->64: k_conv_wgrad_bf16<1, 32, 1>", "k_softmax_ce"],
    "halo-0-lds": ["6x10x64->32 epi 0 pooled-in: k_conv3x3_halo_f32<16, 32>, 4 items", "6x10x32->64 pooled-dZ: k_wgrad3x3_halo_f32<16>, 4 chunks x 2 tiles",
                   "12x20x3->32 pooled-dZ: k_conv1_wgrad_f32<3, 8>, 12 chunks"],
    "halo-1-lds": ["4x4x64->32 epi 0 pooled-in: k_conv3x3_halo_f32<8, 32>, 2 items", "8x8x32->32 epi 3 pooled-in: k_conv3x3_halo_f32<8, 32>, 2 items",
                   "8x8x32->32 pooled-dZ: k_wgrad3x3_halo_f32<8>, 2 chunks x 1 tiles", "8x8x1->32: k_conv1_wgrad_f32<1, 8>, 2 chunks"],
    "halo-5-lds": ["14x6x32->64 epi 0 pooled-in: k_conv3x3_halo_f32<8, 64>, 8 items", "14x6x64->32 pooled-dZ: k_wgrad3x3_halo_f32<8>, 8 chunks x 2 tiles",
                   "28x12x1->64 pooled-dZ: k_conv1_wgrad_f32<1, 16>, 32 chunks"],
    "convnet-0-auto": ["4x4x64->32 epi 0: k_conv_fwd<3, tile, 32> split-K 4", "k_pool_bwd", "k_head_f32", "8x8x3->32 pooled-dZ: k_conv1_wgrad_f32<3, 8>, 2 chunks"],
    "convnet-1-auto": ["6x6x32->32 epi 3: k_conv_fwd<3, tile, 32> split-K 2", "k_pool_bwd", "6x6x1->32: k_conv_wgrad<3, gather, 32>, 1 chunks", "k_softmax_ce"],
    "convnet-2-auto": ["k_head_f32, 4 workgroups", "4x8x3->64: k_conv_wgrad<3, gather, 64>, 4 chunks", "k_pool_bwd"],
    "convnet-3-auto": ["8x8x32->32 pooled-dZ: k_wgrad3x3_halo_f32<8>, 2 chunks x 1 tiles"],
    "convnet-4-auto": ["2x2x256->256 epi 3: k_conv_fwd<3, tile, 64> split-K 18", "4x4x128->64 epi 0: k_conv_fwd<3, tile, 64> split-K 9", "k_pool_bwd",
                       "8x8x64->64: k_wgrad3x3_halo_f32<8>, 2 chunks x 4 tiles", "2x2x256->256: k_conv_wgrad<3, tile, 32>, 1 chunks"],
    "mnist-b8-fp32": ["14x14x64->32 epi 0: k_conv_fwd<3, tile, 32> split-K 4", "14x14x32->64: k_wgrad3x3_halo_f32<16>, 16 chunks x 2 tiles",
                      "28x28x1->32 pooled-dZ: k_conv1_wgrad_f32<1, 16>, 64 chunks", "1x1x3136->128: k_conv_wgrad<1, tile, 32>", "k_head_f32"],
    "mnist-b8-bf16": ["14x14x64->32 epi 0: k_conv_fwd_bf16<3, tile, 32> split-K 4", "14x14x32->64: k_wgrad3x3_halo_bf16<32, 64>, 2 chunks x 1 tiles",
                      "1x1x3136->128: k_conv_wgrad_bf16<1, 32, 2>", "k_head_f32"],
    "mnist-b8-bf16_stored": ["14x14x64->32 epi 0 pooled-in: k_conv3x3_halo_bf16p, 16 items", "14x14x32->64 pooled-dZ: k_wgrad3x3_halo_bf16<32, 64>, 2 chunks x 1 tiles",
                             "bf16 output map"],
    "cifar-b8-fp32": ["8x8x128->64 epi 0: k_conv_fwd<3, tile, 64> split-K 9", "8x8x64->128: k_wgrad3x3_halo_f32<8>, 4 chunks x 8 tiles",
                      "16x16x32->64: k_wgrad3x3_halo_f32<16>, 16 chunks x 2 tiles", "32x32x3->32 pooled-dZ: k_conv1_wgrad_f32<3, 16>, 64 chunks", "k_head_f32"],
    "cifar-b8-bf16": ["8x8x128->64 epi 0: k_conv_fwd_bf16<3, tile, 64> split-K 9", "8x8x64->128: k_wgrad3x3_halo_bf16<64, 64>, 1 chunks x 2 tiles",
                      "1x1x2048->256: k_conv_wgrad_bf16<1, 32, 4>"],
    "cifar-b8-bf16_stored": ["8x8x128->64 epi 0 pooled-in: k_conv3x3_halo_bf16p, 8 items", "16x16x64->32 epi 0 pooled-in: k_conv3x3_halo_bf16p, 16 items",
                             "16x16x32->64 pooled-dZ: k_wgrad3x3_halo_bf16<32, 64>, 2 chunks x 1 tiles"],
    "soft-fused-head": ["k_head_f32"], "soft-plain-head": ["dense 1x1x32->32 epi 1: k_conv_fwd<1, tile, 32>"],
})
BACKWARD_LINES.update({f"xcd-remap-fp32-b{B}": [f"4x8x3->32: k_conv_wgrad<3, gather, 32>, {c} chunks", f"4x8x32->64: k_conv_wgrad<3, tile, 32>, {c} chunks"]
                       for B, c in ((4, 1), (16, 4), (32, 8))})
BACKWARD_LINES.update({f"xcd-remap-bf16-b{B}": [f"4x8x3->32: k_conv_wgrad<3, gather, 32>, {c} chunks", f"4x8x32->64: k_conv_wgrad_bf16<3, 32, 3>, {c} chunks"]
                       for B, c in ((4, 1), (16, 4), (32, 8))})

def _backward_cases():
    looping = [Back("fp32-16wide", _W4, "fp32", "lds", {}), Back("fp32-8wide-pairs", _P8, "fp32", "lds", {}), Back("bf16-1cb-reload", _W4, "bf16", "auto", {}),
               Back("stored-1cb", _S8, "bf16_stored", "auto", {"bf16_1cb": 1}), Back("stored-pipelined", _S8, "bf16_stored", "auto", {"bf16_1cb": 0}),
               Back("bf16-pipelined-3-column-blocks", _PL32, "bf16", "auto", {})]
    cases = list(looping)
    cases += [c._replace(id=f"{c.id}-{s}slots", slots=s) for c in looping for s in (2, 3)]
    cases += [
        # weight-gradient chunks of several pixel blocks, one chunk shorter than the others
        Back("wg16-ragged", at(_F.WG16, 4), "fp32", "lds", {"wgh_f32_target": 7}), Back("wg8-ragged", at(_F.WG8, 4), "fp32", "lds", {"wgh_f32_target": 7}),
        Back("wg-first-layer", at(_F.WG_FIRST, 64), "fp32", "lds", {}), Back("wg-first-layer-ragged", _WG_FIRST40, "fp32", "lds", {}), Back("wg-stored-2-chunks", at(_F.WG_STORED, 4), "bf16_stored", "auto", {}),
    ]
    cases += [Back(f"xcd-remap-fp32-b{B}", _F._flat48(B), "fp32", "gemm", _REMAP16) for B in (4, 16, 32)]
    cases += [Back(f"xcd-remap-bf16-b{B}", _F._flat48(B), "bf16", "auto", _REMAP16H) for B in (4, 16, 32)]
    cases += [
        Back("bf16-not-pipelined", _F.BF16_HALO, "bf16", "auto", {"bf16_pipe": 0}), Back("bf16-not-pipelined-plain", _PL32, "bf16", "auto", {"bf16_pipe": 0}), Back("bf16-plain-b16-split-k", _PL16, "bf16", "auto", {}),
        Back("bf16-no-lds-tiling", _F.BF16_HALO, "bf16", "auto", {"halo": 0}), Back("bf16-implicit-gemm-wgrad", _F.BF16_HALO, "bf16", "auto", {"halo_wgrad": 0}),
        Back("fp32-implicit-gemm-wgrad", _W4, "fp32", "lds", {"halo_wgrad": 0}), Back("fp32-unfused-pool-bwd", _W4, "fp32", "lds", {"fuse_pool_bwd": 0}),
        Back("fp32-64wide-wgrad", _F.WIDTHS64, "fp32", "gemm", {"wgf_policy": 0}), Back("bf16-64wide-wgrad", _F.WIDTHS64, "bf16", "auto", {"wgb_policy": 0, "halo_wgrad": 0}),
        Back("fp32-dense-nk", _F.DENSE_NK, "fp32", "auto", {"head": 0}), Back("bf16-dense-nk", _F.DENSE_NK, "bf16", "auto", {"head": 0}),
    ]
    cases += [Back(f"halo-{i}-lds", at(HALO_NETS[i], B), "fp32", "lds", {}) for i, B in ((0, 4), (1, 4), (5, 8))]
    cases += [Back(f"convnet-{i}-auto", at(CONVNET_NETS[i], B), "fp32", "auto", {}) for i, B in enumerate((4, 4, 128, 4, 4))]
    cases += [Back(f"{name}-b8-{p}", at(spec, 8), p, "auto", {}) for name, spec in (("mnist", MNIST), ("cifar", CIFAR)) for p in MODES]
    cases += [Back("soft-fused-head", SOFT8, "fp32", "auto", {}, extra="soft"), Back("soft-plain-head", SOFT8, "fp32", "auto", {"head": 0}, extra="soft")]
    extras = {"fp32-16wide": "sgd", "bf16-1cb-reload": "sgd", "stored-pipelined": "sgd", "mnist-b8-fp32": "ema", "cifar-b8-bf16_stored": "ema",
              "cifar-b8-bf16": "accum", "halo-5-lds": "accum"}
    return [c._replace(extra=extras.get(c.id, c.extra), lines=BACKWARD_LINES.get(c.id, [])) for c in cases]


BACKWARD_CASES = _backward_cases()
