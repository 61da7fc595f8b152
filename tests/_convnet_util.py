"""What the Track X test files (tests/test_convnet_*.py, tests/test_gpu_convnet*.py) share: the net specs, the optimiser triples, net
construction, device plumbing, the host restatements several files use, the checks and the CPU fixtures.  A new Track X test file starts
from here; a helper only one file needs stays in that file.  Not a test file and not a conftest: pytest does not rewrite `assert` here, so
every assert carries its message."""
import os

import numpy as np
import pytest
from _clip_ref import clip_coef

from oracle import convnet_oracle as co

HEADER = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "rcn_hipx.h")      # Track X's public header

# ---- net specs: (input shape, layers, batch) ---------------------------------------------------------------------------------------------
FUSED_HEAD = ((8, 8, 3), (("conv", 32), ("pool",), ("conv", 64), ("pool",), ("dense_relu", 32), ("dense", 10)), 5)
# padded class columns, one chunk per job; E = 36: the scalar path of a uint8 set
PLAIN_HEAD = ((6, 6, 1), (("conv", 32), ("conv", 32), ("pool",), ("dense", 7)), 3)
# 16 chunks in the first layer's job: reduce_all_body's GR > 1 / threadIdx.x < EL branch and its i < jb.n edge; bf16 storage covers it
POOL_PAIRS = ((16, 16, 3), (("conv", 32), ("pool",), ("conv", 64), ("pool",), ("dense_relu", 128), ("dense", 10)), 64)
ODD_WIDTH = ((5, 7, 1), (("conv", 32), ("dense", 6)), 4)                                            # E = 35: element by element for fp32 too
# BASELINE.json configs[2] and [4], the shapes bench_convnet.py times
CIFAR = ((32, 32, 3), (("conv", 32), ("pool",), ("conv", 64), ("pool",), ("conv", 128), ("pool",), ("dense_relu", 256), ("dense", 10)), 512)
MNIST = ((28, 28, 1), (("conv", 32), ("pool",), ("conv", 64), ("pool",), ("dense_relu", 128), ("dense", 10)), 4096)

# the nets of tests/test_gpu_convnet.py ("auto" tiling: implicit GEMM, split-K, k_pool_fwd)
CONVNET_NETS = [
    FUSED_HEAD,
    PLAIN_HEAD,
    ((4, 8, 3), (("conv", 64), ("pool",), ("dense_relu", 64), ("dense_relu", 32), ("dense", 3)), 130),
    ((8, 8, 32), (("conv", 32), ("pool",), ("dense", 10)), 4),
    # the layer stack of the synthetic 224x224x3 config (BASELINE configs[3]) at 16x16: 8 conv layers, pool after each pair
    ((16, 16, 3), (("conv", 32), ("conv", 32), ("pool",), ("conv", 64), ("conv", 64), ("pool",), ("conv", 128), ("conv", 128), ("pool",),
                   ("conv", 256), ("conv", 256), ("pool",), ("dense", 10)), 3),
]
# ... and of its bf16-operand test: the third one twice as wide
CONVNET_BF16_NETS = [CONVNET_NETS[0], CONVNET_NETS[1], ((4, 8, 3), (("conv", 128), ("pool",), ("dense_relu", 128), ("dense_relu", 32), ("dense", 3)), 130),
                     CONVNET_NETS[4]]
# the nets of tests/test_gpu_convnet_halo.py (tiling "lds"), chosen for the LDS-tiled kernels' corner cases
HALO_NETS = [
    # 8 x 16 blocks, maps 12 x 20 and 6 x 10 (partly empty blocks), first layer RGB + fused pool, 32 -> 64 + fused pool
    ((12, 20, 3), (("conv", 32), ("pool",), ("conv", 64), ("pool",), ("dense", 10)), 3),
    # 8 x 8 blocks of two images, odd batch; 1-channel first layer WITHOUT a pool behind it, conv-conv-pool (gate epilogue + pooled input
    # gradient), a 4 x 4 map
    ((8, 8, 1), (("conv", 32), ("conv", 32), ("pool",), ("conv", 64), ("pool",), ("dense", 7)), 5),
    # 32-channel input: no first-layer kernel; 96 output channels = three 32-wide column blocks; two input-channel blocks behind it
    ((16, 16, 32), (("conv", 64), ("conv", 96), ("pool",), ("conv", 32), ("dense_relu", 32), ("dense", 10)), 2),
    # first layer with two column blocks on an 8-wide map, then 64 -> 32
    ((24, 8, 3), (("conv", 64), ("pool",), ("conv", 32), ("pool",), ("dense", 4)), 4),
    # a batch of 64 (two workgroups of the fused head, one more hidden dense layer in front of it)
    ((8, 8, 3), (("conv", 32), ("pool",), ("dense_relu", 64), ("dense_relu", 32), ("dense", 10)), 64),
    # the MNIST-shape first layer: ONE channel with the pool right behind it (weight gradient on the 16-row MFMA from a pooled-resolution
    # gradient), 64 filters = two column blocks, a 28 x 12 map (blocks that are not full in either direction), several blocks per chunk
    ((28, 12, 1), (("conv", 64), ("pool",), ("conv", 32), ("pool",), ("dense", 10)), 6),
]

# ---- shared scalars ----------------------------------------------------------------------------------------------------------------------
SCALE, SHIFT = 1.0 / 255.0, -0.1307                     # neither is a power of two: a padded uint8 pixel is fl(fl(0*scale)+shift) != 0
KW = dict(x_scale=SCALE, x_shift=SHIFT)
MU, WD = 0.9, 5e-4
PLAIN, MOMENTUM, NESTEROV = (0.0, 0.0, False), (MU, 0.0, False), (MU, WD, True)      # PLAIN: rcn_hipx_set_sgd's default
INF = float("inf")
LR = 0.05                                               # the step rate of the files that use one rate throughout


# ---- net construction --------------------------------------------------------------------------------------------------------------------
def make_net(spec, precision="fp32", sgd=None, max_batch=None, tiling=None):
    """A ConvNet of spec = (in_shape, layers, B).  precision, sgd and tiling reach the library only where they are not None."""
    from mercer_research_amd.convnet import ConvNet
    in_shape, layers, B = spec
    net = ConvNet(in_shape, layers, max_batch or B)
    if tiling is not None:
        net.set_tiling(tiling)
    if precision is not None:
        net.set_precision(precision)
    if sgd is not None:
        net.set_sgd(*sgd)
    return net


def twins(spec, precision, count=2, sgd=None, seed=1, max_batch=None, configured_first=False):
    """`count` nets with the same parameters, precision and optimiser: each twin is built and given the first one's parameters in turn,
    and the optimiser is set last.  configured_first: every net is built with its optimiser before the first is initialised."""
    if configured_first:
        nets = [make_net(spec, precision, sgd, max_batch) for _ in range(count)]
        nets[0].init_params(seed)
        for n in nets[1:]:
            n.set_params(nets[0].get_params())
        return nets
    nets = [make_net(spec, precision, max_batch=max_batch)]
    nets[0].init_params(seed)
    for _ in range(count - 1):
        nets.append(make_net(spec, precision, max_batch=max_batch))
        nets[-1].set_params(nets[0].get_params())
    if sgd is not None:
        for n in nets:
            n.set_sgd(*sgd)
    return nets


# ---- device plumbing ---------------------------------------------------------------------------------------------------------------------
def sync():
    import torch
    torch.cuda.synchronize()


def dev(net, a):
    t = net.to_device(a)
    sync()
    return t


def zeros(net, n):
    import torch
    t = torch.zeros(n, dtype=torch.float32, device=net.device)
    sync()
    return t


def random_set(net, spec, n, seed=0, u8=False):
    in_shape, layers, _ = spec
    rng = np.random.default_rng(seed)
    X = rng.integers(0, 256, (n,) + in_shape).astype(np.uint8) if u8 else rng.standard_normal((n,) + in_shape).astype(np.float32)
    y = rng.integers(0, layers[-1][1], n).astype(np.int32)
    return dev(net, X), dev(net, y)


def batch(net, spec, seed=0):
    in_shape, layers, B = spec
    rng = np.random.default_rng(seed)
    x = net.to_device(rng.standard_normal((B,) + in_shape).astype(np.float32))
    y = net.to_device(rng.integers(0, layers[-1][1], B).astype(np.int32))
    net.synchronize()
    return x, y


def batches(net, spec, n, seed=0):
    """n batches drawn one after the other from ONE generator"""
    in_shape, layers, B = spec
    rng = np.random.default_rng(seed)
    out = [(net.to_device(rng.standard_normal((B,) + in_shape).astype(np.float32)), net.to_device(rng.integers(0, layers[-1][1], B).astype(np.int32)))
           for _ in range(n)]
    net.synchronize()
    return out


def batches_by_seed(net, spec, k, seed=20):
    """k batches, batch j from a generator of its own: batch(net, spec, seed + j)"""
    return [batch(net, spec, seed + j) for j in range(k)]


def mix_records(net, rows):
    """rows of (blend, weight, y0, y1, x0, x1) as a MIX_DTYPE array and as the device tensor train_epoch and gather_mix read"""
    from mercer_research_amd.convnet import MIX_DTYPE
    rec = np.array([tuple(r) for r in rows], dtype=MIX_DTYPE)
    t = net.mix_to_device(rec)
    sync()
    return rec, t


def step(net, x, y, lr, loss=None):
    import torch
    with torch.cuda.stream(net.stream):
        net.train_step(x, y, lr, loss)
    net.synchronize()


def epoch(net, *args, **kw):
    import torch
    with torch.cuda.stream(net.stream):
        net.train_epoch(*args, **kw)
    net.synchronize()


def grad(net, x, y, p=None):
    """the padded gradient (device tensor, host array) of `net` at parameters p (None: its own)"""
    import torch
    if p is not None:
        net.set_params(p)
    with torch.cuda.stream(net.stream):
        g = net.gradients(x, y)
    net.synchronize()
    return g, g.cpu().numpy()


# ---- host restatements -------------------------------------------------------------------------------------------------------------------
def widen(stored):
    """What the gather makes of stored values: fp32 as it is; uint8 as fl(fl(u8 * scale) + shift), two roundings, built with torch."""
    import torch
    if stored.dtype != np.uint8:
        return stored
    t = torch.from_numpy(np.ascontiguousarray(stored)).float() * torch.tensor(SCALE, dtype=torch.float32)
    return (t.float() + torch.tensor(SHIFT, dtype=torch.float32)).numpy()


def oracle_params(rng, in_shape, layers):
    """He-scaled weights, then biases, drawn from rng in that order: (ws, bs, flat, w32, b32) -- the f64 draws, their flat vector, and the
    values the device holds (rounded to float32) as f64 for the oracle"""
    shapes = co.param_shapes(in_shape, layers)
    ws = [rng.standard_normal(k) * np.sqrt(2.0 / k[0]) for k, _ in shapes]
    bs = [rng.standard_normal(n) * 0.1 for _, n in shapes]
    w32 = [w.astype(np.float32).astype(np.float64) for w in ws]
    b32 = [b.astype(np.float32).astype(np.float64) for b in bs]
    return ws, bs, co.flatten(ws, bs), w32, b32


# ---- checks ------------------------------------------------------------------------------------------------------------------------------
def close(a, b, rtol=2e-4, tag=""):
    """tests/test_gpu_convnet.py's rule, fp32 MFMA against f64: |d| <= rtol * max(1e-3, max |ref|) + 1e-6, printing the figure first;
    returns |d| / allowance"""
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    scale = max(1e-3, float(np.abs(b).max()))
    d = float(np.abs(a - b).max())
    print(f"{tag + ': ' if tag else ''}max |d| = {d:.3e} scale = {scale:.3e} rtol = {rtol} used = {d / (rtol * scale + 1e-6):.3f}")
    assert d <= rtol * scale + 1e-6, (tag, d, scale, rtol)
    return d / (rtol * scale + 1e-6)


def tensor_slices(in_shape, layers):
    """every layer's (weights, biases) as slices of the logical flat layout"""
    slices, o = [], 0
    for (k, c), nb in co.param_shapes(in_shape, layers):
        slices.append((slice(o, o + k * c), slice(o + k * c, o + k * c + nb)))
        o += k * c + nb
    return slices


def close_per_tensor(got_logical, ref, in_shape, layers, rtol=2e-4, on_global_scale=()):
    """`close` on every layer's weights and on every layer's biases, each at ITS OWN scale: a tensor's scale is at most the whole
    vector's, so this asks no less than close(got_logical, ref, rtol).  Prints and returns the worst |d| / (rtol * scale + 1e-6).
    on_global_scale: (layer, "weights" | "biases") pairs held at the whole vector's scale instead -- what close(got_logical, ref, rtol)
    asks of them; the caller says why."""
    got, ref = np.asarray(got_logical, dtype=np.float64).ravel(), np.asarray(ref, dtype=np.float64).ravel()
    slices = tensor_slices(in_shape, layers)
    assert got.size == ref.size == slices[-1][1].stop, (got.size, ref.size, slices[-1][1].stop)
    whole = max(1e-3, float(np.abs(ref).max()))
    worst = 0.0
    for li, pair in enumerate(slices):
        for name, s in zip(("weights", "biases"), pair):
            if (li, name) in on_global_scale:
                d = float(np.abs(got[s] - ref[s]).max())
                print(f"layer {li} {name}: max |d| = {d} at the whole vector's scale = {whole} (its own: {float(np.abs(ref[s]).max())}) rtol = {rtol}")
                assert d <= rtol * whole + 1e-6, (li, name, d, whole)
                continue
            worst = max(worst, float(np.abs(got[s] - ref[s]).max()) / (rtol * max(1e-3, float(np.abs(ref[s]).max())) + 1e-6))
            print(f"layer {li} {name}: ", end="")
            close(got[s], ref[s], rtol)
    print("worst per-tensor |d| / allowance =", worst)
    return worst


def bits(a):
    a = np.ascontiguousarray(a)
    assert a.dtype == np.float32, a.dtype
    return a.view(np.uint32)


def same_bits(a, b):
    """equal uint32 patterns (+0 is not -0) and no NaN: what np.array_equal and a comparison of the patterns both accept"""
    a, b = np.asarray(a), np.asarray(b)
    return np.array_equal(bits(a), bits(b)) and not np.isnan(a).any()


def same_state(a, b):
    return same_bits(a.get_params(), b.get_params()) and same_bits(a.get_velocity(), b.get_velocity())


def check_norm(tag, norm_dev, coef_dev, norm_ref, max_norm):
    """the device's coef is clip_coef(norm_dev, max_norm) bit for bit; norm_dev is within one float32 ulp of the restatement's norm (the
    double square root's last bit on the device is the one thing the restatement cannot promise)"""
    norm_dev, coef_dev = np.float32(norm_dev), np.float32(coef_dev)
    print(f"{tag}: norm_dev {norm_dev!r} restatement {norm_ref!r} {'exact' if norm_dev == norm_ref else 'one ulp off'}; coef {coef_dev!r}")
    assert np.array_equal(coef_dev.view(np.uint32), clip_coef(norm_dev, max_norm).view(np.uint32)), (tag, coef_dev, clip_coef(norm_dev, max_norm))
    assert abs(float(norm_dev) - float(norm_ref)) <= float(np.spacing(norm_ref)), (tag, norm_dev, norm_ref)


# ---- CPU side ----------------------------------------------------------------------------------------------------------------------------
def plan_lines(text):
    """the launches of a plan text: every non-empty line after the heading"""
    return [l.strip() for l in text.splitlines()[1:] if l.strip()]


@pytest.fixture(scope="module")
def libx():
    from mercer_research_amd import build as hipbuild, convnet
    hipbuild.build_x()
    return convnet.load()


@pytest.fixture(scope="module", name="convnet")
def convnet_built():
    """the convnet module with its library built, not loaded"""
    from mercer_research_amd import build as hipbuild, convnet
    hipbuild.build_x()
    return convnet


@pytest.fixture(scope="module", name="convnet")
def convnet_loaded():
    """the convnet module with its library built and loaded"""
    from mercer_research_amd import build as hipbuild, convnet
    hipbuild.build_x()
    convnet.load()
    return convnet
