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
             bit (tests/test_convnet_exact_nets.py); the others are the mutants a test on such a net has to tell from it."""
import functools
from collections import namedtuple
from types import SimpleNamespace

import _forms_cases
import numpy as np
from _convnet_util import CONVNET_BF16_NETS, CONVNET_NETS, FUSED_HEAD, HALO_NETS, PLAIN_HEAD, POOL_PAIRS

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


def walk(x, T, ws, bs, layers, operand="f64", stored=False, tie="first", gate=">"):
    """(loss, logits, gws, gbs) for a dense target T [B, C]: tests/_mix_ref.soft_loss_and_grads, and with a one-hot T the oracle's
    loss_and_grads, restated with the pooling rule and the ReLU gate as flags.  gate ">=" lets the gradient through where the
    pre-activation is exactly 0; tie "last" routes a window's gradient to the last of its equal maxima."""
    assert tie in ("first", "last") and gate in (">", ">="), (tie, gate)
    logits, cache = _forward(x, ws, bs, layers, operand, stored, tie)
    open_ = (lambda y, z: y > 0) if gate == ">" else (lambda y, z: z >= 0)
    B = logits.shape[0]
    z = logits - logits.max(axis=1, keepdims=True)
    p = np.exp(z); p /= p.sum(axis=1, keepdims=True)
    T = np.asarray(T, dtype=np.float64)
    with np.errstate(divide="ignore", invalid="ignore"):
        terms = np.where(T != 0, T * np.log(p), 0.0)
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
            dz = (d * open_(y, pre)).reshape(N * H * W, -1)
            small = cols.shape[1] <= 32
            gws[pi] = cols.T @ dz if small else _op(cols, operand).T @ _op(dz, operand); gbs[pi] = dz.sum(axis=0)
            dcols = (_op(dz, operand) @ _op(ws[pi], operand).T).reshape(N, H, W, 9, C)
            dxp = np.zeros((N, H + 2, W + 2, C))
            t = 0
            for kh in range(3):
                for kw in range(3):
                    dxp[:, kh:kh + H, kw:kw + W, :] += dcols[:, :, :, t, :]; t += 1
            d = dxp[:, 1:-1, 1:-1, :]
            pi -= 1
        else:
            kind, f, y, shp, pre = c
            dz = d * open_(y, pre) if kind == "dense_relu" else d
            op = "f64" if (bi == 0 and head32) else operand
            gws[pi] = _op(f, op).T @ _op(dz, op); gbs[pi] = dz.sum(axis=0)
            d = (_op(dz, op) @ _op(ws[pi], op).T).reshape(shp)
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
