"""GPU parity tests (run with -m gpu on an MI355X): the HIP path, called through the C ABI, against the CPU oracle on
identical inputs; against the committed golden vectors; and, at the BASELINE.json sizes, through size-independent
properties.  Tolerances:
  * operators / raw features: bit-exact (f64 in the reference's summation order; integer-valued features)
  * f64 context dense path: <= 1e-11 relative (only the summation order differs from the per-sample reference loop)
  * f32 context dense path: activations abs <= 2e-6; one-step parameters |d| <= 1e-5*|ref| + 1e-6; loss rel <= 1e-5
"""
import os

import numpy as np
import pytest
from _rcn_util import amd, oracle_global_epochs, spawn_ranks  # noqa: F401  (amd: a fixture)

from oracle.rcn_oracle import (DEFAULT_LAYERS, LAYER_CONV, LAYER_POOL, PAD_NONE, PAD_SAME, POOL_MAX, one_hot,
                               synthetic_images, synthetic_params)

pytestmark = pytest.mark.gpu

F32_ACT_ATOL = 2e-6
F32_PARAM_RTOL, F32_PARAM_ATOL = 1e-5, 1e-6
F64_RTOL = 1e-11


def _layers(amd, spec):
    out = []
    for kind, arg in spec:
        out.append(amd.RCNLayer.Convolve2D(amd.Padding(arg)) if kind == LAYER_CONV else amd.RCNLayer.Pool2D(amd.Pooling(arg)))
    return out


def _mk(amd, dims, dtype, layers=DEFAULT_LAYERS, shape=(28, 28), path=0):
    r = amd.RCN(dims[-1], _layers(amd, layers), dims[1:-1], input_shape=shape, dtype=dtype)
    r.set_dense_path(path)      # 0 auto, 1 sample-tile kernels (dense.hpp), 2 feature-sliced pipeline (dense_pipe.hpp)
    return r


# ----------------------------------------------------------------------------------------------------- operators

@pytest.mark.parametrize("shape", [(3, 3), (5, 6), (7, 3), (28, 28), (30, 30), (9, 31), (64, 48)])
def test_operators_bit_exact(amd, oracle, shape):
    rng = np.random.default_rng(sum(shape))
    ints = rng.integers(0, 256, shape).astype(np.float64)
    reals = rng.standard_normal(shape) * 100
    for m in (ints, reals):
        for pad in (PAD_NONE, PAD_SAME):
            for op in range(4):
                assert np.array_equal(amd.convolve_2d_separated(m, amd.SeparableOperator(op), amd.Padding(pad)),
                                      oracle.convolve_2d_separated(m, op, pad))
            for ks in ((3, 3), (1, 3), (3, 1), (1, 1)):
                k = rng.standard_normal(ks)
                assert np.array_equal(amd.convolve_2d(m, k, amd.Padding(pad)), oracle.convolve_2d(m, k, pad))
            assert np.array_equal(amd.pool_2d(m, amd.Padding(pad), amd.Pooling.MAX), oracle.pool_2d(m, pad, POOL_MAX))
        assert np.array_equal(amd.relu(m - 50), oracle.relu(m - 50))
    k5 = rng.standard_normal((5, 5))
    if shape[0] >= 5 and shape[1] >= 5:
        assert np.array_equal(amd.convolve_2d(reals, k5, amd.Padding.NONE), oracle.convolve_2d(reals, k5, PAD_NONE))


def test_operators_random_shapes_agree_with_oracle_including_panics(amd, oracle):
    """150 random (matrix shape, kernel shape, padding) draws: wherever the oracle's restatement of the reference panics
    (utils/kernel.rs:123-135, 154-158, 199-201, 246-251) the library returns the shape error, and everywhere else the result is
    bit-identical -- ragged, tiny and non-square shapes included."""
    from oracle.rcn_oracle import OracleError
    rng = np.random.default_rng(2024)
    n_ok = n_panic = 0
    for _ in range(150):
        R, Cc = int(rng.integers(1, 40)), int(rng.integers(1, 40))
        m = np.round(rng.standard_normal((R, Cc)) * 50)
        kr, kc = int(rng.integers(1, 7)), int(rng.integers(1, 7))
        k = np.round(rng.standard_normal((kr, kc)) * 3)
        pad = int(rng.integers(0, 2))
        cases = [(lambda: amd.convolve_2d(m, k, amd.Padding(pad)), lambda: oracle.convolve_2d(m, k, pad)),
                 (lambda: amd.convolve_2d_separated(m, amd.SeparableOperator(int(rng.integers(0, 4))), amd.Padding(pad)), None),
                 (lambda: amd.pool_2d(m, amd.Padding(pad), amd.Pooling.MAX), lambda: oracle.pool_2d(m, pad, POOL_MAX))]
        op = int(rng.integers(0, 4))
        cases[1] = (lambda: amd.convolve_2d_separated(m, amd.SeparableOperator(op), amd.Padding(pad)), lambda: oracle.convolve_2d_separated(m, op, pad))
        for g, c in cases:
            try:
                want = c()
            except OracleError:
                with pytest.raises(amd.RcnPanic):
                    g()
                n_panic += 1
                continue
            assert np.array_equal(g(), want)
            n_ok += 1
    assert n_ok > 200 and n_panic > 40, (n_ok, n_panic)


def test_operator_reference_kats(amd):
    """utils/kernel.rs:436-441 (identity Same conv on 0..900) through the HIP path."""
    m = np.arange(900, dtype=np.float64).reshape(30, 30)
    k = np.array([[0, 0, 0], [0, 1, 0], [0, 0, 0]], dtype=np.float64)
    assert np.array_equal(amd.convolve_2d(m, k, amd.Padding.SAME), m)


def test_operator_batched(amd, oracle):
    rng = np.random.default_rng(5)
    ms = rng.integers(0, 256, (7, 12, 9)).astype(np.float64)
    got = amd.convolve_2d_separated(ms, amd.SeparableOperator.LEFT, amd.Padding.SAME)
    for i in range(7):
        assert np.array_equal(got[i], oracle.convolve_2d_separated(ms[i], 2, PAD_SAME))
    got = amd.pool_2d(ms, amd.Padding.SAME, amd.Pooling.MAX)
    for i in range(7):
        assert np.array_equal(got[i], oracle.pool_2d(ms[i], PAD_SAME, POOL_MAX))


def test_operator_panics(amd):
    m = np.ones((8, 8))
    for ks in ((2, 2), (2, 3), (5, 5), (5, 1), (1, 5)):
        with pytest.raises(amd.RcnPanic):
            amd.convolve_2d(m, np.ones(ks), amd.Padding.SAME)
    with pytest.raises(amd.RcnPanic):
        amd.convolve_2d(np.ones((2, 2)), np.ones((3, 3)), amd.Padding.NONE)
    with pytest.raises(amd.RcnPanic):
        amd.convolve_2d_separated(np.ones((2, 8)), amd.SeparableOperator.TOP, amd.Padding.SAME)
    with pytest.raises(amd.RcnPanic):
        amd.pool_2d(np.ones((1, 8)), amd.Padding.SAME, amd.Pooling.MAX)
    with pytest.raises(amd.RcnPanic):
        amd.pool_2d(np.ones((4, 4)), amd.Padding.SAME, amd.Pooling.AVERAGE)


# ----------------------------------------------------------------------------------------------------- features

@pytest.mark.parametrize("dtype", [0, 1])
def test_features_default_net_bit_exact(amd, oracle, dtype):
    imgs, _ = synthetic_images(96, seed=21)
    imgs[0] = 255                        # saturated image
    imgs[3, ::2] = 255; imgs[3, 1::2] = 0  # stripes: strongest edge responses
    imgs[1] = 0
    imgs[2] = np.random.default_rng(0).integers(0, 256, (28, 28))   # no black border: exercises the Q1 edge columns
    r = _mk(amd, [784, 30, 10], dtype)
    got = r.flatten_feature_set(imgs)
    assert got.shape == (96, 784)
    assert np.array_equal(got, oracle.features(imgs, DEFAULT_LAYERS))
    assert 2040 < got.max() <= 16320.0      # bound of SURVEY §8c: 255 * 8^2


@pytest.mark.parametrize("dtype", [1, 0], ids=["f64", "f32"])
def test_features_specialised_and_generic_kernels_agree(amd, oracle, dtype):
    """The fused conv+pool kernel for the default stack (k_features_cpcp) and the generic layer-walking kernel are both
    the reference's flatten_feature_set (rcn.rs:317-356): bit-identical to each other and to the oracle, with and
    without the fused standardisation, on inputs that light every border (quirk Q1) and every pixel individually."""
    import torch
    from mercer_research_amd.device import DeviceRCN
    rng = np.random.default_rng(99)
    imgs = rng.integers(0, 256, (1200, 28, 28)).astype(np.uint8)
    imgs[0] = 255
    imgs[1] = 0
    imgs[2, ::2] = 255; imgs[2, 1::2] = 0
    imgs[3, :, ::2] = 255; imgs[3, :, 1::2] = 0
    hot = np.zeros((784, 28, 28), np.uint8)                       # one image per single hot pixel
    hot.reshape(784, 784)[np.arange(784), np.arange(784)] = 255
    imgs[100:884] = hot
    ref = oracle.features(imgs, DEFAULT_LAYERS)
    d = DeviceRCN(dtype=dtype)
    dev = d.to_device(imgs)

    def feats(x, **kw):
        t = d.features(x, **kw)
        d.synchronize()                 # the kernels run on the context's stream, .cpu() on torch's
        return t.cpu().numpy()

    fast = feats(dev)
    d.set_feature_kernel(1)
    slow = feats(dev)
    assert np.array_equal(fast, ref) and np.array_equal(slow, ref)
    assert not np.signbit(fast).any()                             # relu(-x) of x == 0 is +0, as in the reference
    d.rcn.scale_set = (37.5, 211.0)
    slow_s = feats(dev, standardize=True)
    d.set_feature_kernel(0)
    fast_s = feats(dev, standardize=True)
    assert np.array_equal(fast_s, slow_s)
    want = oracle.standardize(ref, 37.5, 211.0)
    np.testing.assert_allclose(fast_s, want, rtol=1e-12 if dtype == 1 else 1e-6, atol=0 if dtype == 1 else 1e-7)
    # an image count that is not a multiple of the grid, and a single image
    for n in (1, 4097):
        big = np.tile(imgs, (4, 1, 1))[:n]
        got = feats(d.to_device(big))
        assert np.array_equal(got, np.tile(ref, (4, 1))[:n])
    d.rcn.close()


def test_fused_standardisation_is_the_division_bit_for_bit_under_random_scales(amd):
    """The specialised f32 feature kernel standardises with a corrected reciprocal product that the host admits only after
    checking it against the division (rcn.rs:407-412) for every value a feature can take; the generic kernel always
    divides.  Under random scales -- including ones the check must refuse (sd <= 0) and extreme ones -- the two kernels'
    outputs carry the same bits, signs of zero included, and every attainable feature value is exercised."""
    from mercer_research_amd.device import DeviceRCN
    rng = np.random.default_rng(2024)
    imgs = rng.integers(0, 256, (600, 28, 28)).astype(np.uint8)
    imgs[:200] = (rng.random((200, 28, 28)) < 0.5) * 255             # saturated edges: the largest responses (up to 4080)
    d = DeviceRCN(dtype=0)
    dev = d.to_device(imgs)

    def bits(kernel):
        d.set_feature_kernel(kernel)
        t = d.features(dev, standardize=True)
        d.synchronize()
        return t.cpu().numpy().view(np.uint32)

    d.set_feature_kernel(0)
    raw = d.features(dev); d.synchronize()
    assert raw.max().item() > 3000
    scales = [(1.0, 1.0), (0.0, 1.0), (33.3184, 78.5675), (-5.0, 3.0), (12.5, -7.0), (100.0, 1e-30), (1e30, 3.0), (7.0, 1e30),
              (0.1, 0.3), (4080.0, 1.0 / 3.0)]
    scales += [(float(rng.uniform(0, 400)), float(rng.uniform(1e-3, 900))) for _ in range(30)]
    for mean, sd in scales:
        d.rcn.scale_set = (mean, sd)
        fast, slow = bits(0), bits(1)
        assert np.array_equal(fast, slow), (mean, sd)
    d.rcn.close()


@pytest.mark.parametrize("spec,shape", [
    (((LAYER_CONV, PAD_NONE), (LAYER_POOL, POOL_MAX)), (9, 11)),
    (((LAYER_CONV, PAD_SAME), (LAYER_POOL, POOL_MAX)), (9, 11)),
    (((LAYER_POOL, POOL_MAX), (LAYER_CONV, PAD_SAME), (LAYER_POOL, POOL_MAX)), (9, 11)),
    (((LAYER_CONV, PAD_NONE), (LAYER_POOL, POOL_MAX), (LAYER_CONV, PAD_SAME), (LAYER_POOL, POOL_MAX)), (32, 32)),
    (((LAYER_CONV, PAD_SAME), (LAYER_POOL, POOL_MAX), (LAYER_CONV, PAD_SAME), (LAYER_POOL, POOL_MAX),
      (LAYER_CONV, PAD_SAME), (LAYER_POOL, POOL_MAX)), (28, 28)),
])
def test_features_other_stacks_bit_exact(amd, oracle, spec, shape):
    rng = np.random.default_rng(len(spec))
    imgs = rng.integers(0, 256, (5,) + shape).astype(np.uint8)
    F = oracle.feature_len(shape[0], shape[1], spec)
    r = amd.RCN(10, _layers(amd, spec), [4], input_shape=shape, dtype=1)
    assert r.feature_len == F
    assert np.array_equal(r.flatten_feature_set(imgs), oracle.features(imgs, spec))


def test_features_random_stacks_agree_with_oracle_including_panics(amd, oracle):
    """40 random conv/pool stacks (up to 5 layers, Padding::None / Same mixed, pools anywhere) on random non-square inputs:
    where the oracle's flatten_feature_set panics the context cannot be created, elsewhere the features are bit-identical
    and the feature length matches."""
    from oracle.rcn_oracle import OracleError
    rng = np.random.default_rng(77)
    n_ok = n_panic = 0
    for _ in range(40):
        H, W = int(rng.integers(2, 34)), int(rng.integers(2, 34))
        spec = []
        for _l in range(int(rng.integers(1, 6))):
            if rng.random() < 0.6 and sum(1 for k, _a in spec if k == LAYER_CONV) < 3:
                spec.append((LAYER_CONV, int(rng.integers(0, 2))))
            else:
                spec.append((LAYER_POOL, POOL_MAX))
        spec = tuple(spec)
        imgs = rng.integers(0, 256, (3, H, W)).astype(np.uint8)
        try:
            want = oracle.features(imgs, spec)
        except OracleError:
            with pytest.raises(amd.RcnPanic):
                amd.RCN(10, _layers(amd, spec), [4], input_shape=(H, W), dtype=1)
            n_panic += 1
            continue
        r = amd.RCN(10, _layers(amd, spec), [4], input_shape=(H, W), dtype=1)
        assert r.feature_len == want.shape[1]
        assert np.array_equal(r.flatten_feature_set(imgs), want), (spec, H, W)
        r.close()
        n_ok += 1
    assert n_ok >= 20 and n_panic >= 3, (n_ok, n_panic)


def test_features_maps_larger_than_lds_spill_to_global_memory(amd, oracle):
    """Three un-pooled Same convolutions on a 48x40 input: 64 maps of 1920 values = 480 KB per image and buffer, three times
    what a CU's LDS holds.  The reference has no such limit (rcn.rs:317-356); the generic feature kernel then keeps its two
    ping-pong buffers in global memory -- same code, bit-identical result."""
    spec = ((LAYER_CONV, PAD_SAME), (LAYER_CONV, PAD_SAME), (LAYER_CONV, PAD_SAME), (LAYER_POOL, POOL_MAX))
    imgs = np.random.default_rng(8).integers(0, 256, (5, 48, 40)).astype(np.uint8)
    want = oracle.features(imgs, spec)
    for dtype in (1, 0):
        r = amd.RCN(10, _layers(amd, spec), [4], input_shape=(48, 40), dtype=dtype)
        assert r.feature_len == want.shape[1] == 64 * 24 * 20
        assert np.array_equal(r.flatten_feature_set(imgs), want)
        r.close()


def test_feature_stack_errors(amd):
    P, L = amd.Padding, amd.RCNLayer
    # fan-in formula 4^c/2^p*l != feature length (rcn.rs:443): RCN::new and the feature path work, train panics in gemv
    r = amd.RCN(10, [L.Convolve2D(P.SAME), L.Convolve2D(P.SAME), L.Pool2D(amd.Pooling.MAX)], [4], input_shape=(12, 12))
    assert r.feature_len == 16 * 36 and r.flatten_feature_set(np.zeros((12, 12), np.uint8)).shape == (576,)
    with pytest.raises(amd.RcnPanic):
        r.train_batch(np.zeros((2, 576)), np.zeros((2, 10)), 3.0)
    with pytest.raises(amd.RcnPanic):
        r.load_weights_and_bias(1)
    with pytest.raises(amd.RcnPanic):          # conv on a map smaller than 3x3
        amd.RCN(10, [L.Convolve2D(P.NONE), L.Pool2D(amd.Pooling.MAX)], [4], input_shape=(2, 9))
    with pytest.raises(amd.RcnPanic):          # Pooling::Average -> "Not implemented"
        amd.RCN(10, [L.Convolve2D(P.SAME), L.Pool2D(amd.Pooling.AVERAGE)], [4], input_shape=(8, 8))
    r = amd.RCN(10, [L.Pool2D(amd.Pooling.MAX)], [4], input_shape=(8, 8))     # no conv layer: empty feature vector
    assert r.feature_len == 0 and r.flatten_feature_set(np.zeros((3, 8, 8), np.uint8)).shape == (3, 0)
    with pytest.raises(amd.RcnPanic):
        r.load_weights_and_bias(1)


@pytest.mark.parametrize("dtype", [0, 1])
def test_gen_scales_and_standardize(amd, oracle, dtype):
    imgs, _ = synthetic_images(200, seed=4)
    f = oracle.features(imgs, DEFAULT_LAYERS)
    r = _mk(amd, [784, 30, 10], dtype)
    m, s = r.gen_scales(f)
    mo, so = oracle.gen_scales(f)
    assert abs(m - mo) <= 1e-12 * abs(mo) and abs(s - so) <= 1e-12 * abs(so)
    assert r.scale_set == (m, s)                                   # gen_scales overwrites scale_set (rcn.rs:249-250)
    r.scale_set = (mo, so)
    assert np.array_equal(r.standardize(f), oracle.standardize(f, mo, so))


def test_classify_images_path(amd, oracle):
    """RCN::classify (rcn.rs:82-98): features -> standardise with scale_set -> classify_test -> last-max arg-max."""
    imgs, _ = synthetic_images(40, seed=9)
    ws, bs = synthetic_params([784, 30, 10], seed=3)
    ws = [w * 0.05 for w in ws]
    for dtype in (0, 1):
        r = _mk(amd, [784, 30, 10], dtype)
        r.set_params(ws, bs)
        f = oracle.features(imgs, DEFAULT_LAYERS)
        mo, so = oracle.gen_scales(f)
        r.scale_set = (mo, so)
        out = oracle.classify_test(ws, bs, oracle.standardize(f, mo, so))
        srt = np.sort(out, axis=1)
        clear = (srt[:, -1] - srt[:, -2]) > 1e-4                     # skip near-ties in the f32 context
        expect = np.array([oracle.classify_argmax(o) for o in out])
        got = r.classify_many(imgs)
        assert clear.sum() > 20 and np.array_equal(got[clear], expect[clear])
        assert r.classify(imgs[int(np.argmax(clear))]) == expect[int(np.argmax(clear))]


@pytest.mark.parametrize("dims", [[784, 30, 10], [784, 10, 10, 10], [784, 40, 7], [784, 64, 10]],
                         ids=["default", "suite-variant", "widest-fused", "fallback-3-launch"])
def test_classify_single_launch_kernel_matches_staged_path_and_oracle(amd, oracle, dims):
    """The one-launch serving kernel (serve.hpp: features -> standardise -> all layers -> arg-max) must return the classes
    of the staged path (feature kernel, forward kernel, arg-max kernel) and of the oracle's RCN::classify (rcn.rs:82-98),
    for single requests and for small batches; nets it does not cover take the staged path."""
    imgs, _ = synthetic_images(70, seed=19)
    ws, bs = synthetic_params(dims, seed=4)
    ws = [w * 0.05 for w in ws]
    f = oracle.features(imgs, DEFAULT_LAYERS)
    mo, so = oracle.gen_scales(f)
    out = oracle.classify_test(ws, bs, oracle.standardize(f, mo, so))
    srt = np.sort(out, axis=1)
    expect = np.array([oracle.classify_argmax(o) for o in out])
    for dtype in (1, 0):
        clear = (srt[:, -1] - srt[:, -2]) > (1e-9 if dtype == 1 else 1e-4)
        r = _mk(amd, dims, dtype)
        r.set_params(ws, bs)
        r.scale_set = (mo, so)
        fused = r.classify_many(imgs)
        singles = np.array([r.classify(imgs[i]) for i in range(12)])
        r.set_feature_kernel(1)                                       # forces the generic feature kernel and the staged path
        staged = r.classify_many(imgs)
        assert clear.sum() > 35
        assert np.array_equal(fused[clear], expect[clear]) and np.array_equal(staged[clear], expect[clear])
        assert np.array_equal(singles[clear[:12]], expect[:12][clear[:12]])
        r.close()


# ----------------------------------------------------------------------------------------------------- dense path

def _dense_case(dims, B, seed, wscale=1.0):
    rng = np.random.default_rng(seed)
    ws, bs = synthetic_params(dims, seed=seed)
    ws = [w * wscale for w in ws]
    X = np.maximum(rng.standard_normal((B, dims[0])), 0.0)
    Y = one_hot(rng.integers(0, dims[-1], B), dims[-1])
    return ws, bs, X, Y


def _check_params(got, ref, dtype):
    for a, b in zip(got, ref):
        if dtype == 1:
            np.testing.assert_allclose(a, b, rtol=F64_RTOL, atol=1e-13)
        else:
            assert np.all(np.abs(a - b) <= F32_PARAM_RTOL * np.abs(b) + F32_PARAM_ATOL), float(np.abs(a - b).max())


@pytest.mark.parametrize("path", [1, 2])
@pytest.mark.parametrize("dtype", [0, 1])
@pytest.mark.parametrize("dims,B", [([784, 30, 10], 32), ([784, 30, 10], 10), ([784, 10, 10, 10], 10), ([784, 30, 10], 1),
                                    ([784, 30, 10], 17), ([784, 30, 10], 256), ([784, 12, 7], 512), ([16, 5, 3], 4), ([100, 70, 33, 40, 10], 33), ([48, 8, 6, 10], 255)])
def test_train_batch_matches_oracle(amd, oracle, dims, B, dtype, path):
    # wscale keeps |z| moderate so that sigmoid' is not identically zero (un-scaled N(0,1) init saturates)
    ws, bs, X, Y = _dense_case(dims, B, seed=B + len(dims), wscale=0.1)
    r = _dense_rcn(amd, dims, dtype, path)
    r.set_params(ws, bs)
    out = r.classify_test(X)
    ref_out = oracle.classify_test(ws, bs, X)
    assert np.abs(out - ref_out).max() <= (1e-13 if dtype == 1 else F32_ACT_ATOL)
    loss = r.train_batch(X, Y, 3.0, want_loss=True)
    nw, nb, cost = oracle.train_batch(ws, bs, X, Y, 3.0)
    assert abs(loss - cost) <= (1e-12 if dtype == 1 else 1e-5) * max(cost, 1e-3)
    gw, gb = r.get_params()
    _check_params(gw + gb, nw + nb, dtype)


def test_train_batch_random_layer_stacks_match_oracle(amd, oracle):
    """25 random dense stacks -- 1 to 3 hidden layers of 1..70 units, 2..16 classes, F in {16, 24, 48, 100, 784}, batch 1..300 --
    through whichever kernels the library picks (path 0) and through each forced path that applies, in the f64 context: forward
    outputs, cost and every updated parameter against the oracle's sequential train_batch (rcn.rs:176-314)."""
    rng = np.random.default_rng(909)
    ran = 0
    for case in range(25):
        F = int(rng.choice([16, 24, 48, 100, 784]))
        hidden = [int(rng.integers(1, 71)) for _ in range(int(rng.integers(1, 4)))]
        dims = [F] + hidden + [int(rng.integers(2, 17))]
        B = int(rng.choice([1, 2, 7, 32, 33, 100, 256, 300]))
        ws, bs, X, Y = _dense_case(dims, B, seed=1000 + case, wscale=0.1)
        ref_out = oracle.classify_test(ws, bs, X)
        nw, nb, cost = oracle.train_batch(ws, bs, X, Y, 3.0)
        for path in (0, 1, 2):
            r = _dense_rcn(amd, dims, 1, 0)
            try:
                r.set_dense_path(path)
            except amd.RcnPanic:                 # the feature-sliced pipeline needs >= 2 dense layers whose tail fits LDS
                r.close()
                continue
            r.set_params(ws, bs)
            assert np.abs(r.classify_test(X) - ref_out).max() <= 1e-13, (dims, B, path)
            loss = r.train_batch(X, Y, 3.0, want_loss=True)
            assert abs(loss - cost) <= 1e-12 * max(cost, 1e-3), (dims, B, path)
            gw, gb = r.get_params()
            _check_params(gw + gb, nw + nb, 1)
            r.close()
            ran += 1
    assert ran >= 60


@pytest.mark.parametrize("dtype", [1, 0], ids=["f64", "f32"])
def test_wide_hidden_layers_run_layer_by_layer(amd, oracle, dtype):
    """Hidden layers too wide for the LDS-resident forward kernel (about 512 units in f32, 128 in f64): the reference has no
    width limit (RCN::new never fails), so the step then runs layer by layer on global activations (dense_wide.hpp).  Forward,
    cost, one train_batch and the batched evaluation against the oracle."""
    dims = [784, 700, 260, 10]
    B = 37
    ws, bs, X, Y = _dense_case(dims, B, seed=5150, wscale=0.02)
    r = _dense_rcn(amd, dims, dtype, 0)
    r.set_params(ws, bs)
    out = r.classify_test(X)
    ref_out = oracle.classify_test(ws, bs, X)
    assert np.abs(out - ref_out).max() <= (1e-12 if dtype == 1 else 5e-6)
    loss = r.train_batch(X, Y, 3.0, want_loss=True)
    nw, nb, cost = oracle.train_batch(ws, bs, X, Y, 3.0)
    assert abs(loss - cost) <= (1e-11 if dtype == 1 else 1e-4) * max(cost, 1e-3)
    gw, gb = r.get_params()
    if dtype == 1:
        _check_params(gw + gb, nw + nb, 1)
    else:
        for a, b in zip(gw + gb, nw + nb):
            assert np.all(np.abs(a - b) <= 1e-4 * np.abs(b) + 1e-5)
    r.close()


def _dense_rcn(amd, dims, dtype, path=0):
    """An RCN whose conv/pool stack yields exactly dims[0] features: conv(Same) + pool(Max) on a 2a x 2b image gives
    4*a*b features and satisfies the reference's fan-in formula (one conv, one pool; rcn.rs:443)."""
    if dims[0] == 784:
        return _mk(amd, dims, dtype, path=path)
    F = dims[0]
    assert F % 4 == 0, "dense test sizes must be 4*a*b with a,b >= 2"
    q = F // 4
    a = next(d for d in range(int(np.sqrt(q)), 1, -1) if q % d == 0)
    b = q // a
    assert a >= 2 and b >= 2
    r = amd.RCN(dims[-1], _layers(amd, ((LAYER_CONV, PAD_SAME), (LAYER_POOL, POOL_MAX))), dims[1:-1], input_shape=(2 * a, 2 * b), dtype=dtype)
    assert r.feature_len == F
    r.set_dense_path(path)
    return r


@pytest.mark.parametrize("path", [1, 2])
@pytest.mark.parametrize("dtype", [0, 1])
def test_unscaled_n01_init_default_net(amd, oracle, dtype, path):
    """The reference's actual init (N(0,1), un-scaled, rcn.rs:500-523) on the synthetic MNIST-shape workload."""
    imgs, labels = synthetic_images(64, seed=11)
    f = oracle.features(imgs, DEFAULT_LAYERS)
    m, s = oracle.gen_scales(f)
    X, Y = oracle.standardize(f, m, s), one_hot(labels)
    ws, bs = synthetic_params([784, 30, 10], seed=42)
    r = _mk(amd, [784, 30, 10], dtype, path=path)
    r.set_params(ws, bs)
    loss = r.train_batch(X, Y, 3.0, want_loss=True)
    nw, nb, cost = oracle.train_batch(ws, bs, X, Y, 3.0)
    assert abs(loss - cost) <= (1e-12 if dtype == 1 else 2e-5) * cost
    gw, gb = r.get_params()
    if dtype == 1:
        _check_params(gw + gb, nw + nb, dtype)
    else:
        # |z| ~ sqrt(784)*|x| here: f32 rounding of z (~1e-5 abs) moves saturated sigmoids by up to ~1e-5 relative
        for a, b in zip(gw + gb, nw + nb):
            assert np.all(np.abs(a - b) <= 1e-4 * np.abs(b) + 1e-5)


def test_golden_dense_fixtures(amd, golden_dir):
    g = np.load(os.path.join(golden_dir, "dense.npz"))
    for name in ("tiny", "mid3", "one"):
        dims = [int(d) for d in g[f"{name}_dims"]]
        L = len(dims) - 1
        ws = [g[f"{name}_W{l}"] for l in range(L)]
        bs = [g[f"{name}_b{l}"] for l in range(L)]
        for dtype in (0, 1):
            r = _dense_rcn(amd, dims, dtype)
            r.set_params(ws, bs)
            out = r.classify_test(g[f"{name}_X"])
            assert np.abs(out - g[f"{name}_out"]).max() <= (1e-13 if dtype == 1 else F32_ACT_ATOL)
            loss = r.train_batch(g[f"{name}_X"], g[f"{name}_Y"], float(g[f"{name}_eta"]), want_loss=True)
            assert abs(loss - float(g[f"{name}_cost"])) <= (1e-12 if dtype == 1 else 1e-5) * float(g[f"{name}_cost"])
            gw, gb = r.get_params()
            _check_params(gw + gb, [g[f"{name}_nW{l}"] for l in range(L)] + [g[f"{name}_nb{l}"] for l in range(L)], dtype)


def test_golden_mnist_fixture_end_to_end(amd, golden_dir):
    """u8 images -> HIP features -> HIP gen_scales/standardise -> HIP train_batch, against the committed numbers."""
    g = np.load(os.path.join(golden_dir, "dense.npz"))
    imgs, labels = synthetic_images(32, seed=11)
    ws, bs = synthetic_params([784, 30, 10], seed=42)
    r = _mk(amd, [784, 30, 10], 1)
    r.set_params(ws, bs)
    X, Y = r.load_data(imgs, labels)
    assert np.abs(r.classify_test(X) - g["mnist_out"]).max() <= 1e-12
    loss = r.train_batch(X, Y, 3.0, want_loss=True)
    assert abs(loss - float(g["mnist_cost"])) <= 1e-11 * float(g["mnist_cost"])
    gw, gb = r.get_params()
    np.testing.assert_allclose(gb[0], g["mnist_nb0"], rtol=1e-10, atol=1e-13)
    np.testing.assert_allclose(gb[1], g["mnist_nb1"], rtol=1e-10, atol=1e-13)
    np.testing.assert_allclose(gw[1], g["mnist_nW1"], rtol=1e-10, atol=1e-13)
    np.testing.assert_allclose(gw[0].ravel(order="F")[::37], g["mnist_nW0_strided"], rtol=1e-10, atol=1e-13)


def test_golden_feature_fixtures(amd, golden_dir):
    g = np.load(os.path.join(golden_dir, "features.npz"))
    r = _mk(amd, [784, 30, 10], 0)
    assert np.array_equal(r.flatten_feature_set(g["imgs"]), g["feats"])
    for k in ("conv_none_pool", "conv_conv_pool", "pool_first"):
        spec = [tuple(int(v) for v in row) for row in g[f"layers_{k}"]]
        rr = amd.RCN(10, _layers(amd, spec), [4], input_shape=(9, 11), dtype=1)
        assert np.array_equal(rr.flatten_feature_set(g["small"]), g[f"small_{k}"])


def test_evaluate_semantics(amd, oracle):
    ws, bs, X, _ = _dense_case([784, 30, 10], 300, seed=2, wscale=0.05)
    r = _mk(amd, [784, 30, 10], 1)
    r.set_params(ws, bs)
    out = oracle.classify_test(ws, bs, X)
    Y = one_hot(out.argmax(axis=1))
    Y[::3] = np.roll(Y[::3], 1, axis=1)                       # make a third of the expectations wrong
    expect = sum(oracle.eval_accept(o, y) for o, y in zip(out, Y))
    assert r.evaluate(X, Y) == expect and 150 < expect < 300
    # a constant network ties every class: one-hot(v == max) is all ones -> never equals a one-hot label (rcn.rs:155)
    r.set_params([w * 0 for w in ws], [b * 0 for b in bs])
    assert r.evaluate(X, Y) == 0


# ----------------------------------------------------------------------------------------------------- device-resident paths

@pytest.mark.parametrize("path", [1, 2])
@pytest.mark.parametrize("dtype", [0, 1])
def test_epoch_graph_matches_sequential_oracle(amd, oracle, dtype, path):
    import torch
    from mercer_research_amd.device import DeviceRCN
    B, nb, N = 32, 6, 256
    ws, bs, X, Y = _dense_case([784, 30, 10], N, seed=77, wscale=0.1)
    d = DeviceRCN(dtype=dtype)
    d.set_dense_path(path)
    d.set_params(ws, bs)
    Xd, Yd = d.to_device(X, d.tdtype), d.to_device(Y, d.tdtype)
    perm = np.random.default_rng(1).permutation(N).astype(np.int32)
    permd = d.to_device(perm)
    loss = d.empty(nb)
    d.synchronize()
    d.train_epoch(Xd, Yd, permd, B, nb, 3.0, loss)
    d.train_epoch(Xd, Yd, permd, B, nb, 3.0, loss)             # replay of the cached graph: a second epoch
    gw, gb = d.get_params()
    losses = loss.cpu().numpy()
    rw, rb = ws, bs
    costs = []
    for _ in range(2):
        costs = []
        for j in range(nb):
            sel = perm[j * B:(j + 1) * B]
            rw, rb, c = oracle.train_batch(rw, rb, X[sel], Y[sel], 3.0)
            costs.append(c)
    if dtype == 1:
        _check_params(gw + gb, rw + rb, 1)
        np.testing.assert_allclose(losses, costs, rtol=1e-10)
    else:
        for a, b in zip(gw + gb, rw + rb):                      # 12 chained f32 steps
            assert np.all(np.abs(a - b) <= 2e-4 * np.abs(b) + 2e-5)
        np.testing.assert_allclose(losses, costs, rtol=1e-3)
    # identity order (perm = NULL) == chunks_exact over the stored order
    d.set_params(ws, bs)
    d.train_epoch(Xd, Yd, None, B, 2, 3.0, None)
    gw, gb = d.get_params()
    rw, rb, _ = oracle.train_batch(ws, bs, X[:B], Y[:B], 3.0)
    rw, rb, _ = oracle.train_batch(rw, rb, X[B:2 * B], Y[B:2 * B], 3.0)
    if dtype == 1:
        _check_params(gw + gb, rw + rb, 1)


def test_removed_dense_paths_are_refused_and_the_context_still_trains(amd, oracle):
    """Dense paths 3 (one resident kernel per epoch segment) and 4 (one launch per step) were removed: set_dense_path refuses them
    with RCN_HIP_ERR_UNSUPPORTED and leaves the context on the path it had -- here the two-kernel pipeline, still the oracle's loop."""
    from mercer_research_amd.device import DeviceRCN
    B, nb, N = 256, 3, 768
    ws, bs, X, Y = _dense_case([784, 30, 10], N, seed=83, wscale=0.1)
    d = DeviceRCN(dtype=0)
    d.set_dense_path(2)
    for mode in (3, 4):
        with pytest.raises(amd.RcnHipError) as e:
            d.set_dense_path(mode)
        assert e.value.status == -3 and "removed" in str(e.value), str(e.value)      # RCN_HIP_ERR_UNSUPPORTED
    d.set_params(ws, bs)
    Xd, Yd = d.to_device(X, d.tdtype), d.to_device(Y, d.tdtype)
    perm = np.random.default_rng(6).permutation(N).astype(np.int32)
    loss = d.empty(nb)
    d.train_epoch(Xd, Yd, d.to_device(perm), B, nb, 3.0, loss)
    gw, gb = d.get_params()
    rw, rb, costs = ws, bs, []
    for j in range(nb):
        sel = perm[j * B:(j + 1) * B]
        rw, rb, c = oracle.train_batch(rw, rb, X[sel], Y[sel], 3.0)
        costs.append(c)
    for a, b in zip(gw + gb, rw + rb):
        assert np.all(np.abs(a - b) <= 2e-4 * np.abs(b) + 2e-5)
    np.testing.assert_allclose(loss.cpu().numpy(), costs, rtol=1e-3)
    d.rcn.close()


@pytest.mark.parametrize("dtype", [1, 0], ids=["f64", "f32"])
def test_native_rccl_epoch_world1_matches_oracle(amd, oracle, dtype):
    """rcn_hip_dp_train_epoch_dev (gradient kernels -> ncclAllReduce -> update, all enqueued natively) with a
    one-rank RCCL communicator must be the reference's sequential train_batch loop (rcn.rs:147-149, 176-223)."""
    from mercer_research_amd.device import DeviceRCN
    B, nb, N = 32, 5, 256
    ws, bs, X, Y = _dense_case([784, 30, 10], N, seed=78, wscale=0.1)
    d = DeviceRCN(dtype=dtype)
    d.set_params(ws, bs)
    assert d.dp_init() == (0, 1)
    assert d.lib.rcn_hip_dp_world(d.ctx) == 1 and d.lib.rcn_hip_dp_rank(d.ctx) == 0
    d.dp_broadcast_params(0)
    Xd, Yd = d.to_device(X, d.tdtype), d.to_device(Y, d.tdtype)
    perm = np.random.default_rng(2).permutation(N).astype(np.int32)
    permd = d.to_device(perm)
    loss = d.empty(nb)
    d.dp_train_epoch(Xd, Yd, permd, B, nb, 3.0, loss)
    gw, gb = d.get_params()
    losses = loss.cpu().numpy()
    rw, rb, costs = ws, bs, []
    for j in range(nb):
        sel = perm[j * B:(j + 1) * B]
        rw, rb, c = oracle.train_batch(rw, rb, X[sel], Y[sel], 3.0)
        costs.append(c)
    if dtype == 1:
        _check_params(gw + gb, rw + rb, 1)
        np.testing.assert_allclose(losses, costs, rtol=1e-10)
    else:
        for a, b in zip(gw + gb, rw + rb):
            assert np.all(np.abs(a - b) <= 2e-4 * np.abs(b) + 2e-5)
        np.testing.assert_allclose(losses, costs, rtol=1e-3)
    # identity order, and the uninitialised / finalised states fail loudly
    d.dp_train_epoch(Xd, Yd, None, B, 2, 3.0, None)
    d.dp_finalize()
    with pytest.raises(Exception):
        d.dp_train_epoch(Xd, Yd, None, B, 1, 3.0, None)
    d.rcn.close()


@pytest.mark.parametrize("dtype,Bs,nb,fused,world", [(1, 16, 4, 1, 2), (0, 16, 4, 1, 2), (1, 256, 3, 0, 2), (0, 256, 3, 0, 2), (1, 256, 3, 1, 2),
                                                      (0, 256, 3, 1, 2), (1, 256, 2, 1, 4), (0, 16, 3, 1, 4), (1, 256, 2, 0, 4), (1, 256, 2, 1, -2), (1, 256, 2, 0, -2),
                                                      (0, 64, 5, 2, 2), (0, 64, 3, 2, -2)],
                         ids=["f64-sample-tile", "f32-sample-tile", "f64-pipeline-3-kernels", "f32-pipeline-3-kernels",
                              "f64-pipeline-exchange-in-kernel", "f32-pipeline-exchange-in-kernel", "f64-4-ranks-exchange-in-kernel",
                              "f32-4-ranks-sample-tile", "f64-4-ranks-3-kernels", "f64-784-12-7-exchange-in-kernel", "f64-784-12-7-3-kernels",
                              "f32-resident-one-xcd-kernel", "f32-784-12-7-resident-one-xcd-kernel"])
def test_peer_allreduce_two_processes_one_gpu(amd, oracle, dtype, Bs, nb, fused, world, tmp_path):
    """The xGMI peer-read all-reduce (csrc/dp_p2p.hpp) between two PROCESSES (hipIpc handles carried by gloo), both on this
    box's one GPU: the known-answer self-test is exact, both replicas end bit-identical, and two epochs of the sharded
    loop equal the oracle's sequential train_batch on the concatenated global batches."""
    # shard batch 16: sample-tile gradient kernels + k_p2p_allreduce; shard batch 256: the feature-sliced pipeline with the
    # exchange either in a third kernel (k_p2_dp_grad / k_p2_dp_apply) or inside the gradient kernel (k_p2_dp_fused)
    # (2 or 4 rank processes: with the test runner that stays within the box's limit of 6 processes on the GPU)
    dims = [784, 30, 10]
    if world < 0:                                                    # a second shape class member: one tail tile, odd sizes
        dims, world = [784, 12, 7], -world
    # fused == 2: the resident one-XCD kernel with the exchange inside it (dense_xcd.hpp, DP form: reduce-scatter + all-gather on pushed
    # words, dp_push.hpp), every rank on an XCD of its own (tests/_p2p_worker.py).  At a shard of 64 samples: a resident launch's
    # blocks -- also the 224 idle ones -- all ask for the kernel's LDS, 66 KB at this size, so a rank's idle blocks fit beside the
    # workers of the peer whose XCD they land on.  At a shard of 256 (148 KB, a whole CU) they cannot: they queue behind the peer's
    # workers, which wait for this rank's workers queued behind them -- by construction, on ONE shared device only; a GPU per rank
    # has no peer workers on it (round 2 ran that case opt-in and saw it pass once and time out otherwise).
    resident = fused == 2
    fused = 1 if resident else fused
    # (no case name: the worker is started as it always was here, and takes its "default")
    Xs, Ys, _ = spawn_ranks(tmp_path, world, dtype, None, {"RCN_HIP_DP_FUSED": str(fused), "RCN_HIP_XCD": "1" if resident else "0"}, dims=dims, Bs=Bs, nb=nb)
    outs = [np.load(tmp_path / f"out{r}.npz") for r in range(world)]
    for o in outs:
        assert int(o["bad"]) == 0 and int(o["timed_out"]) == 0 and int(o["active"]) == (2 if fused else 1)
        assert int(o["resident"]) == int(resident), "the data-parallel epoch did not run on the kernel this case is about"
    for r in range(1, world):
        for k in ("w0", "w1", "b0", "b1", "loss"):
            assert np.array_equal(outs[0][k], outs[r][k]), (r, k)     # rank-order sums: replicas are bit-identical
    rw, rb, costs = oracle_global_epochs(oracle, dims, Xs, Ys, Bs, nb)
    got = [outs[0]["w0"], outs[0]["w1"], outs[0]["b0"], outs[0]["b1"]]
    want = [rw[0], rw[1], rb[0], rb[1]]
    if dtype == 1:
        _check_params(got, want, 1)
        np.testing.assert_allclose(outs[0]["loss"], costs, rtol=1e-10)
    else:
        # f32.  Measured on MI355X over the thirteen cases of this test (2 x nb = 4..10 chained steps; printed below): parameters within
        # 3.9e-7 x (|ref| + 0.1), costs within 1.6e-7 relative of the f64 oracle.  Asserted at ten times that -- tighter than SURVEY
        # 8(c)'s one-step tolerance (1e-5 x |ref| + 1e-6); round 2 asserted 2e-4 x |ref| + 2e-5 and 1e-3 on the costs here.
        dev_p = max(float(np.max(np.abs(a - b) / (np.abs(b) + 0.1))) for a, b in zip(got, want))
        dev_c = float(np.max(np.abs(outs[0]["loss"] - costs) / np.abs(costs)))
        print(f"MEASURED two-process f32 {dims} Bs={Bs} world={world} fused={fused}: params {dev_p:.3e} (relative to |ref| + 0.1), costs {dev_c:.3e}")
        for a, b in zip(got, want):
            assert np.all(np.abs(a - b) <= 4e-6 * (np.abs(b) + 0.1)), float(np.max(np.abs(a - b) / (np.abs(b) + 0.1)))
        np.testing.assert_allclose(outs[0]["loss"], costs, rtol=2e-6)


def test_peer_allreduce_bootstrap_over_rccl_world1(amd, oracle, monkeypatch):
    """rcn_hip_dp_init's own set-up of the peer all-reduce (export -> ncclAllGather of the handles -> attach -> known-answer
    vote) forced on at world size 1: every line of the bootstrap except the peer mappings runs, and the epoch loop on the
    peer-read kernel is the oracle's loop."""
    from mercer_research_amd.device import DeviceRCN
    monkeypatch.setenv("RCN_HIP_DP_P2P", "2")
    B, nb, N = 32, 5, 256
    ws, bs, X, Y = _dense_case([784, 30, 10], N, seed=79, wscale=0.1)
    d = DeviceRCN(dtype=1)
    d.set_params(ws, bs)
    assert d.dp_init() == (0, 1) and d.dp_p2p_active()
    Xd, Yd = d.to_device(X, d.tdtype), d.to_device(Y, d.tdtype)
    loss = d.empty(nb)
    d.dp_train_epoch(Xd, Yd, None, B, nb, 3.0, loss)
    gw, gb = d.get_params()
    rw, rb, costs = ws, bs, []
    for j in range(nb):
        rw, rb, c = oracle.train_batch(rw, rb, X[j * B:(j + 1) * B], Y[j * B:(j + 1) * B], 3.0)
        costs.append(c)
    _check_params(gw + gb, rw + rb, 1)
    np.testing.assert_allclose(loss.cpu().numpy(), costs, rtol=1e-10)
    d.set_option("dp_p2p", 0)                         # (the environment only seeds the option when the context is created)
    d.dp_init()
    assert not d.dp_p2p_active()
    d.dp_finalize()
    d.rcn.close()


@pytest.mark.parametrize("B", [256, 512])
def test_two_kernel_pipeline_graph_replays_track_the_oracle(amd, oracle, B, monkeypatch):
    """dense path 2 at the specialised shape (f32, dense_p2.hpp: k_p2_a / k_p2_b with the operand-fragment image rebuilt by every
    captured call) is the oracle's sequential train_batch loop, per-step costs included: shuffled and in stored order, across segment
    boundaries of the epoch image, over repeated replays of one captured graph and from u8 pictures."""
    from mercer_research_amd.device import DeviceRCN
    monkeypatch.setenv("RCN_HIP_PACK_SEGMENT_BYTES", str(3 * 49 * B * 16 * 4))      # 3 batches per segment
    nb, N = 7, 8 * B
    imgs, labels = synthetic_images(N, seed=31)
    ws, bs = synthetic_params([784, 30, 10], seed=13)
    ws = [w * 0.1 for w in ws]
    perm = np.random.default_rng(8).permutation(N).astype(np.int32)
    d = DeviceRCN(dtype=0)
    d.set_dense_path(2)
    d.set_params(ws, bs)
    dev = d.to_device(imgs)
    Yd = d.to_device(one_hot(labels, 10), d.tdtype)
    mean, sd = d.gen_scales(d.features(dev))
    d.rcn.scale_set = (mean, sd)
    Xs = d.features(dev, standardize=True)
    permd = d.to_device(perm)
    loss = d.empty(nb)
    costs = []
    for _ in range(3):                                               # three replays of the same captured graph
        d.train_epoch(Xs, Yd, permd, B, nb, 3.0, loss)
        d.synchronize()
        costs.append(loss.cpu().numpy().copy())
    d.train_epoch(Xs, Yd, None, B, 2, 3.0, None)                     # stored order, another graph
    d.train_epoch_images(dev, Yd, permd, B, nb, 3.0, loss)           # straight from the pictures
    d.synchronize()
    costs.append(loss.cpu().numpy().copy())
    gw, gb = d.get_params()
    Xh, Yh = Xs.double().cpu().numpy(), one_hot(labels, 10)
    d.rcn.close()
    rw, rb, want = ws, bs, []
    for call in range(4):
        if call == 3:
            for j in range(2):
                rw, rb, _ = oracle.train_batch(rw, rb, Xh[j * B:(j + 1) * B], Yh[j * B:(j + 1) * B], 3.0)
        c = []
        for j in range(nb):
            sel = perm[j * B:(j + 1) * B]
            rw, rb, cj = oracle.train_batch(rw, rb, Xh[sel], Yh[sel], 3.0)
            c.append(cj)
        want.append(c)
    # Measured on MI355X (30 chained f32 steps): parameters within 4.3e-7 x (|ref| + 0.1), costs within 3.1e-7 relative of the f64
    # oracle at B = 256 and 512.  Asserted at about ten times that.
    dev_p = max(float(np.max(np.abs(a - b) / (np.abs(b) + 0.1))) for a, b in zip(gw + gb, rw + rb))
    dev_c = max(float(np.max(np.abs(g - w) / np.abs(w))) for g, w in zip(costs, want))
    print(f"MEASURED path 2 f32 B={B}, 30 chained steps: params {dev_p:.3e} (relative to |ref| + 0.1), costs {dev_c:.3e}")
    for g, w in zip(costs, want):
        np.testing.assert_allclose(g, w, rtol=3e-6)
    for a, b in zip(gw + gb, rw + rb):
        assert np.all(np.abs(a - b) <= 5e-6 * (np.abs(b) + 0.1)), float(np.max(np.abs(a - b) / (np.abs(b) + 0.1)))
    assert np.isfinite(costs[-1]).all() and costs[-1][-1] < costs[0][0]


@pytest.mark.parametrize("dtype", [0, 1], ids=["f32", "f64"])
def test_train_epoch_from_images_equals_features_then_train(amd, oracle, dtype, monkeypatch):
    """rcn_hip_train_epoch_images_dev (u8 pictures -> features -> standardise -> packed epoch image in one kernel per segment,
    then the training steps) must leave exactly the parameters of rcn_hip_features_dev(standardize) + rcn_hip_train_epoch_dev,
    shuffled and in stored order, across a segment boundary of the epoch image, and both equal the oracle's loop."""
    import torch
    from mercer_research_amd.device import DeviceRCN
    monkeypatch.setenv("RCN_HIP_PACK_SEGMENT_BYTES", str(3 * 49 * 256 * 16 * (8 if dtype == 1 else 4)))     # 3 batches per segment
    B, nb, N = 256, 5, 1536
    imgs, labels = synthetic_images(N, seed=23)
    ws, bs = synthetic_params([784, 30, 10], seed=9)
    ws = [w * 0.1 for w in ws]
    res = []
    for images_path in (True, False):
        d = DeviceRCN(dtype=dtype)
        d.set_dense_path(2)
        d.set_params(ws, bs)
        dev = d.to_device(imgs)
        raw = d.features(dev)
        mean, sd = d.gen_scales(raw)                                  # also sets scale_set
        Y = d.to_device(one_hot(labels), d.tdtype)
        perm = d.to_device(np.random.default_rng(4).permutation(N).astype(np.int32))
        loss = d.empty(nb)
        if images_path:
            d.train_epoch_images(dev, Y, perm, B, nb, 3.0, loss)
            d.train_epoch_images(dev, Y, None, B, 2, 3.0, None)
        else:
            X = d.features(dev, standardize=True)
            d.train_epoch(X, Y, perm, B, nb, 3.0, loss)
            d.train_epoch(X, Y, None, B, 2, 3.0, None)
        gw, gb = d.get_params()
        res.append((gw + gb, loss.cpu().numpy().copy(), (mean, sd)))
        d.rcn.close()
    for a, b in zip(res[0][0], res[1][0]):
        assert np.array_equal(a, b)
    assert np.array_equal(res[0][1], res[1][1])
    # and the oracle's loop on the oracle's features
    f = oracle.features(imgs, DEFAULT_LAYERS)
    mo, so = oracle.gen_scales(f)
    X = oracle.standardize(f, mo, so)
    Yh = one_hot(labels)
    p = np.random.default_rng(4).permutation(N)
    rw, rb = ws, bs
    for j in range(nb):
        sel = p[j * B:(j + 1) * B]
        rw, rb, _ = oracle.train_batch(rw, rb, X[sel], Yh[sel], 3.0)
    for j in range(2):
        rw, rb, _ = oracle.train_batch(rw, rb, X[j * B:(j + 1) * B], Yh[j * B:(j + 1) * B], 3.0)
    tol = (1e-9, 1e-10) if dtype == 1 else (3e-4, 3e-5)
    for a, b in zip(res[0][0], rw + rb):
        assert np.all(np.abs(a - b) <= tol[0] * np.abs(b) + tol[1])


def test_cached_epoch_graphs_survive_workspace_growth(amd, oracle):
    """A short epoch call, then a longer one (its packed image needs a larger workspace, which moves), then the short shape
    again: the graph cached for the first shape pointed into the old workspace and must not be replayed as is.  Parameters after
    the three calls equal the oracle's sequential loop.  (A use-after-free found by benchmarking with warm-up < timed steps.)"""
    from mercer_research_amd.device import DeviceRCN
    B, N = 256, 5120
    ws, bs, X, Y = _dense_case([784, 30, 10], N, seed=321, wscale=0.1)
    d = DeviceRCN(dtype=1)
    d.set_params(ws, bs)
    Xd, Yd = d.to_device(X, d.tdtype), d.to_device(Y, d.tdtype)
    perm = np.random.default_rng(12).permutation(N).astype(np.int32)
    permd = d.to_device(perm)
    calls = [(0, 2), (2, 17), (0, 2), (5, 9)]                      # (first batch, number of batches)
    rw, rb = ws, bs
    for j0, nb in calls:
        d.train_epoch(Xd, Yd, permd[j0 * B:], B, nb, 3.0, None)
        for j in range(j0, j0 + nb):
            sel = perm[j * B:(j + 1) * B]
            rw, rb, _ = oracle.train_batch(rw, rb, X[sel], Y[sel], 3.0)
    gw, gb = d.get_params()
    _check_params(gw + gb, rw + rb, 1)
    d.rcn.close()


def test_random_call_sequences_track_the_oracle(amd, oracle):
    """40 randomly chosen calls on ONE f64 context -- train_batch and train_epoch at changing batch sizes / lengths / index
    arguments, evaluation and forward calls in between, the dense path switched now and then -- with the oracle stepping the
    same parameters.  Shakes out state that outlives a call (cached graphs, workspaces, packed images)."""
    from mercer_research_amd.device import DeviceRCN
    rng = np.random.default_rng(4242)
    N = 2048
    ws, bs, X, Y = _dense_case([784, 30, 10], N, seed=99, wscale=0.1)
    d = DeviceRCN(dtype=1)
    d.set_params(ws, bs)
    Xd, Yd = d.to_device(X, d.tdtype), d.to_device(Y, d.tdtype)
    rw, rb = ws, bs
    for step in range(40):
        op = rng.choice(["batch", "epoch", "epoch_perm", "eval", "forward", "path"], p=[0.25, 0.2, 0.3, 0.1, 0.1, 0.05])
        if op == "batch":
            B = int(rng.choice([1, 7, 32, 256, 512]))
            j = int(rng.integers(0, N - B))
            d.train_batch(Xd[j:j + B].contiguous(), Yd[j:j + B].contiguous(), 3.0)
            rw, rb, _ = oracle.train_batch(rw, rb, X[j:j + B], Y[j:j + B], 3.0)
        elif op == "epoch":
            B = int(rng.choice([32, 256]))
            nb = int(rng.integers(1, N // B + 1))
            d.train_epoch(Xd, Yd, None, B, nb, 3.0, None)
            for j in range(nb):
                rw, rb, _ = oracle.train_batch(rw, rb, X[j * B:(j + 1) * B], Y[j * B:(j + 1) * B], 3.0)
        elif op == "epoch_perm":
            B = int(rng.choice([16, 256]))
            nb = int(rng.integers(1, N // B + 1))
            perm = rng.permutation(N).astype(np.int32)
            d.train_epoch(Xd, Yd, d.to_device(perm), B, nb, 3.0, None)
            for j in range(nb):
                sel = perm[j * B:(j + 1) * B]
                rw, rb, _ = oracle.train_batch(rw, rb, X[sel], Y[sel], 3.0)
        elif op == "eval":
            n = int(rng.integers(1, N))
            want = int(sum(oracle.eval_accept(o, y) for o, y in zip(oracle.classify_test(rw, rb, X[:n]), Y[:n])))    # rcn.rs:152-157
            got = d.evaluate(Xd[:n].contiguous(), Yd[:n].contiguous())
            assert got == want
        elif op == "forward":
            n = int(rng.integers(1, 300))
            out = d.forward(Xd[:n].contiguous())
            d.synchronize()
            assert np.abs(out.cpu().numpy() - oracle.classify_test(rw, rb, X[:n])).max() <= 1e-9
        else:
            d.set_dense_path(int(rng.choice([0, 1, 2])))
        if op in ("batch", "epoch", "epoch_perm") and step % 5 == 4:
            gw, gb = d.get_params()
            for a, b in zip(gw + gb, rw + rb):
                assert np.all(np.abs(a - b) <= 1e-8 * np.abs(b) + 1e-9), (step, op)
    gw, gb = d.get_params()
    for a, b in zip(gw + gb, rw + rb):
        assert np.all(np.abs(a - b) <= 1e-8 * np.abs(b) + 1e-9)
    d.rcn.close()


@pytest.mark.parametrize("fused", ["1", "0"], ids=["exchange-in-kernel", "3-kernels"])
def test_random_data_parallel_call_sequences_world1(amd, oracle, monkeypatch, fused):
    """The data-parallel loop with the peer exchange forced on at world size 1 (so every kernel, graph and sequence number of the
    multi-GPU path runs): 25 calls of random length and position, some of them the plain single-GPU epoch in between (they share
    the packed-image workspace), tracked by the oracle in f64."""
    from mercer_research_amd.device import DeviceRCN
    monkeypatch.setenv("RCN_HIP_DP_P2P", "2")
    monkeypatch.setenv("RCN_HIP_DP_FUSED", fused)
    rng = np.random.default_rng(777)
    N, B = 8192, 256
    ws, bs, X, Y = _dense_case([784, 30, 10], N, seed=98, wscale=0.1)
    d = DeviceRCN(dtype=1)
    d.set_params(ws, bs)
    d.dp_init()
    assert d.dp_p2p_mode() == (2 if fused == "1" else 1)
    Xd, Yd = d.to_device(X, d.tdtype), d.to_device(Y, d.tdtype)
    perm = rng.permutation(N).astype(np.int32)
    permd = d.to_device(perm)
    rw, rb = ws, bs
    for call in range(25):
        nb = int(rng.integers(1, 25))
        j0 = int(rng.integers(0, N // B - nb + 1))
        use_perm = rng.random() < 0.7
        plain = rng.random() < 0.25
        fn = d.train_epoch if plain else d.dp_train_epoch
        fn(Xd if use_perm else Xd[j0 * B:], Yd if use_perm else Yd[j0 * B:], permd[j0 * B:] if use_perm else None, B, nb, 3.0, None)
        for j in range(j0, j0 + nb):
            sel = perm[j * B:(j + 1) * B] if use_perm else np.arange(j * B, (j + 1) * B)
            rw, rb, _ = oracle.train_batch(rw, rb, X[sel], Y[sel], 3.0)
    gw, gb = d.get_params()
    for a, b in zip(gw + gb, rw + rb):
        assert np.all(np.abs(a - b) <= 1e-8 * np.abs(b) + 1e-9)
    d.dp_finalize()
    d.rcn.close()


def test_data_parallel_halves_equal_full_batch(amd, oracle):
    """Shard gradients + sum + one update == train_batch on the concatenated batch, single GPU."""
    from mercer_research_amd.device import DeviceRCN
    ws, bs, X, Y = _dense_case([784, 30, 10], 64, seed=5, wscale=0.1)
    d = DeviceRCN(dtype=1)
    d.set_params(ws, bs)
    Xd, Yd = d.to_device(X, d.tdtype), d.to_device(Y, d.tdtype)
    d.synchronize()
    g0 = d.batch_gradient(Xd[:32].contiguous(), Yd[:32].contiguous())
    g1 = d.batch_gradient(Xd[32:].contiguous(), Yd[32:].contiguous())
    gfull = d.batch_gradient(Xd, Yd)
    d.synchronize()
    np.testing.assert_allclose((g0 + g1).cpu().numpy(), gfull.cpu().numpy(), rtol=1e-10, atol=1e-13)
    gW, gb, _ = oracle.batch_gradient(ws, bs, X, Y)
    flat = np.concatenate([np.concatenate([w.ravel(order="F"), b]) for w, b in zip(gW, gb)])
    np.testing.assert_allclose(gfull.cpu().numpy(), flat, rtol=1e-10, atol=1e-13)
    d.apply_gradient(g0 + g1, 3.0 / 64)
    gw, gbb = d.get_params()
    nw, nb, _ = oracle.train_batch(ws, bs, X, Y, 3.0)
    _check_params(gw + gbb, nw + nb, 1)
    # params_flat is a live view of the same buffer
    pf = d.params_flat()
    assert pf.numel() == 23860
    np.testing.assert_allclose(pf.cpu().numpy()[:784 * 30], gw[0].ravel(order="F"), rtol=0, atol=0)


@pytest.mark.parametrize("B", [256, 4096])
def test_full_size_properties(amd, B):
    """BASELINE.json sizes (B=256 config 2, B=4096 config 5): additivity of the batch gradient over any split,
    permutation invariance, and zero gradient for a perfectly-fit target -- no oracle needed."""
    import torch
    from mercer_research_amd.device import DeviceRCN
    d = DeviceRCN(dtype=1)
    ws, bs = synthetic_params([784, 30, 10], seed=1)
    d.set_params([w * 0.05 for w in ws], bs)
    imgs, labels = synthetic_images(B, seed=B)
    with torch.cuda.stream(d.stream):
        imgs_d = torch.from_numpy(imgs).to(d.device)
        lab_d = torch.from_numpy(labels).to(d.device)
    X, Y = d.load_data(imgs_d, lab_d)
    with torch.cuda.stream(d.stream):             # torch ops must run on the context's stream to be ordered with our kernels
        full = d.batch_gradient(X, Y).clone()
        cut = B // 4 + 3
        parts = d.batch_gradient(X[:cut].contiguous(), Y[:cut].contiguous()).clone() + d.batch_gradient(X[cut:].contiguous(), Y[cut:].contiguous())
        p = torch.randperm(B, device=d.device)
        permuted = d.batch_gradient(X[p].contiguous(), Y[p].contiguous()).clone()
        fit = d.forward(X)
        zero = d.batch_gradient(X, fit.contiguous())
    d.synchronize()
    scale = full.abs().max().item()
    assert scale > 0
    assert (parts - full).abs().max().item() <= 1e-11 * scale
    assert (permuted - full).abs().max().item() <= 1e-11 * scale
    assert zero.abs().max().item() == 0.0


def test_full_size_feature_properties(amd, oracle):
    """16 384 images (the bench set): device features are integers in range, invariant to batch order, and equal to
    the oracle on a sample."""
    import torch
    from mercer_research_amd.device import DeviceRCN
    d = DeviceRCN(dtype=0)
    imgs, _ = synthetic_images(16384)
    with torch.cuda.stream(d.stream):
        imgs_d = torch.from_numpy(imgs).to(d.device)
        f = d.features(imgs_d)
        idx = torch.randperm(16384, device=d.device)
        f2 = d.features(imgs_d[idx].contiguous())
    d.synchronize()
    assert torch.equal(f[idx], f2)
    assert torch.equal(f, f.round()) and f.min().item() >= 0 and f.max().item() <= 16320
    sel = np.arange(0, 16384, 331)
    assert np.array_equal(f[sel].cpu().numpy().astype(np.float64), oracle.features(imgs[sel], DEFAULT_LAYERS))
    m, s = d.gen_scales(f)
    fo = f.double()
    assert abs(m - fo.mean().item()) <= 1e-9 * m and abs(s - fo.std(unbiased=False).item()) <= 1e-9 * s


def test_cpp_host_mirror_trains_on_gpu(tmp_path):
    """The C++ mirror of RCN::{new, train, classify} (csrc/host/rcn.hpp) end to end: accuracy rises, Average pooling panics."""
    import subprocess
    from mercer_research_amd import _lib
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    exe = tmp_path / "host_demo"
    subprocess.run(["g++", "-std=c++17", "-O2", os.path.join(root, "tests", "cpp", "host_demo.cpp"), "-L" + os.path.dirname(_lib.LIB_PATH),
                    "-lrcn_hip", "-lz", "-Wl,-rpath," + os.path.dirname(_lib.LIB_PATH), "-o", str(exe)], check=True)
    out = subprocess.run([str(exe)], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "Epoch 0:" in out.stdout and "host_demo ok" in out.stdout


def test_long_epoch_call_repacks_in_segments(amd, oracle, monkeypatch):
    """One train_epoch call longer than the packed image's segment (forced small here): the image is re-packed in two
    alternating halves; results must equal sequential oracle steps.  B=256 -> specialised kernels; 3 segments."""
    import torch
    from mercer_research_amd.device import DeviceRCN
    B, nb, N = 256, 5, 1024
    dims = [3136, 30, 10]
    ws, bs = synthetic_params(dims, seed=3)
    ws = [w * 0.05 for w in ws]
    rng = np.random.default_rng(3)
    X = np.maximum(rng.standard_normal((N, dims[0])), 0.0)
    Y = one_hot(rng.integers(0, 10, N), 10)
    layers = [amd.RCNLayer.Convolve2D(amd.Padding.SAME), amd.RCNLayer.Pool2D(amd.Pooling.MAX)]
    monkeypatch.setenv("RCN_HIP_PACK_SEGMENT_BYTES", str(2 * 196 * 256 * 16 * 8))      # two batches per half of the image
    d = DeviceRCN(convpool_cfg=layers, feedforward_cfg=[30], input_shape=(56, 56), dtype=1)
    assert d.F == 3136
    d.set_params(ws, bs)
    Xd, Yd = d.to_device(X, d.tdtype), d.to_device(Y, d.tdtype)
    perm = np.random.default_rng(5).permutation(N).astype(np.int32)
    perm = np.concatenate([perm, perm[::-1]])[: nb * B].copy()
    permd = d.to_device(perm)
    loss = d.empty(nb)
    d.synchronize()
    d.train_epoch(Xd, Yd, permd, B, nb, 1.0, loss)
    gw, gb = d.get_params()
    rw, rb, costs = ws, bs, []
    for j in range(nb):
        sel = perm[j * B:(j + 1) * B]
        rw, rb, c = oracle.train_batch(rw, rb, X[sel], Y[sel], 1.0)
        costs.append(c)
    _check_params(gw + gb, rw + rb, 1)
    np.testing.assert_allclose(loss.cpu().numpy(), costs, rtol=1e-10)
    # the specialised kernels (F = 784) through the same segmented driver, three batches per half, f32
    monkeypatch.setenv("RCN_HIP_PACK_SEGMENT_BYTES", str(3 * 49 * 256 * 16 * 4))
    d2 = DeviceRCN(dtype=0)
    ws2, bs2 = synthetic_params([784, 30, 10], seed=4)
    ws2 = [w * 0.1 for w in ws2]
    d2.set_params(ws2, bs2)
    X2 = X[:, :784].copy()
    X2d, Y2d = d2.to_device(X2, d2.tdtype), d2.to_device(Y, d2.tdtype)
    nb2 = 8
    perm2 = np.concatenate([perm, perm])[: nb2 * B].copy()
    d2.synchronize()
    d2.train_epoch(X2d, Y2d, d2.to_device(perm2), B, nb2, 1.0, None)
    gw, gb = d2.get_params()
    rw, rb = ws2, bs2
    for j in range(nb2):
        sel = perm2[j * B:(j + 1) * B]
        rw, rb, _ = oracle.train_batch(rw, rb, X2[sel], Y[sel], 1.0)
    for a, b in zip(gw + gb, rw + rb):
        assert np.all(np.abs(a - b) <= 1e-4 * np.abs(b) + 1e-5)


def test_device_shuffle_writes_permutations(amd):
    """rcn_hip_shuffle_dev (training_set.shuffle, rcn.rs:146): every pass is a permutation of 0..n-1; passes and seeds differ."""
    import torch
    from mercer_research_amd.device import DeviceRCN
    d = DeviceRCN()
    for n, passes in ((16384, 8), (1000, 3), (7, 5), (1, 2), (65537, 2)):
        perm = torch.full((n * passes,), -1, dtype=torch.int32, device=d.device)
        torch.cuda.synchronize()                         # the fill runs on torch's stream, the shuffle on the context's own
        d.shuffle(perm, n, passes, seed=1234)
        d.synchronize()
        p = perm.cpu().numpy().reshape(passes, n)
        for row in p:
            assert np.array_equal(np.sort(row), np.arange(n))
        if n >= 1000:
            assert not np.array_equal(p[0], p[1]) and not np.array_equal(p[0], np.arange(n))
            assert abs(np.corrcoef(p[0], np.arange(n))[0, 1]) < 0.1          # not an affine/near-identity map
            perm2 = torch.empty_like(perm)
            d.shuffle(perm2, n, passes, seed=1235)
            d.synchronize()
            assert not np.array_equal(perm2.cpu().numpy(), perm.cpu().numpy())


def _write_png_set(root, protos, per_class, rng):
    from mercer_research_amd import png
    for c, proto in enumerate(protos):
        os.makedirs(os.path.join(root, str(c)))
        for i in range(per_class):
            img = proto.copy()
            img[rng.random(img.shape) < 0.12] = 0
            with open(os.path.join(root, str(c), f"{i}.png"), "wb") as f:
                f.write(png.encode_gray(img))


def test_cli_trains_from_png_directories_saves_and_resumes(amd, oracle, tmp_path, capsys):
    """the reference CLI's flow (rcn/src/main.rs:44-79) on PNG directories: load_data front end, epoch lines,
    bincode rcn.bin written; a second run resumes from it ("weights non-empty => skip init", rcn.rs:139-141); the saved
    model classifies a file like RCN::classify and its parameters reproduce the oracle's forward pass."""
    from mercer_research_amd import checkpoint, cli
    rng = np.random.default_rng(3)
    protos = []
    for _ in range(10):
        p = np.zeros((28, 28), dtype=np.uint8)
        p[4:24, 4:24] = np.where(rng.random((20, 20)) < 0.3, rng.integers(80, 256, (20, 20)), 0)
        protos.append(p)
    tr, te, model_path = str(tmp_path / "training"), str(tmp_path / "testing"), str(tmp_path / "rcn.bin")
    _write_png_set(tr, protos, 40, rng)
    _write_png_set(te, protos, 12, rng)
    argv = ["--training-path", tr, "--testing-path", te, "--training-class-size", "40", "--testing-class-size", "12", "-b", "10", "-e", "6",
            "--model-path", model_path, "--seed", "5"]
    assert cli.main(argv) == 0
    out = capsys.readouterr().out.strip().splitlines()
    assert len(out) == 6 and all(l.startswith(f"Epoch {i}: ") and l.endswith("%]") for i, l in enumerate(out))
    acc = [int(l.split(": ")[1].split("/")[0]) for l in out]
    assert out[0].split(": ")[1].split(" ")[0].endswith("/120") and acc[-1] >= 60 and acc[-1] > acc[0]   # un-scaled N(0,1) init learns slowly; chance = 12
    ck = checkpoint.loads(open(model_path, "rb").read())
    assert ck.classes == 10 and ck.convpool_cfg == [(0, 1), (1, 1), (0, 1), (1, 1)] and ck.feedforward_cfg == [30]
    assert [w.shape for w in ck.layer_weights] == [(30, 784), (10, 30)] and ck.training_path == tr
    # resume: the second run starts from the saved weights, so its first epoch is already accurate
    argv2 = ["--training-path", tr, "--testing-path", te, "--training-class-size", "40", "--testing-class-size", "12", "-b", "10", "-e", "1",
             "--model-path", model_path, "--seed", "6"]
    assert cli.main(argv2) == 0
    out2 = capsys.readouterr().out.strip().splitlines()
    assert int(out2[0].split(": ")[1].split("/")[0]) >= acc[-1] - 15     # continues from the saved weights, not from a fresh init
    # the saved model in a fresh context: RCN::classify on a file, and parity of its forward pass with the oracle
    m = checkpoint.load_model(model_path)
    f = os.path.join(te, "7", "0.png")
    ck2 = checkpoint.loads(open(model_path, "rb").read())
    from mercer_research_amd import png as _png
    img = _png.to_pixel_matrix_u8(open(f, "rb").read())
    feats = oracle.features(img[None], DEFAULT_LAYERS)
    x = oracle.standardize(feats, ck2.scale_set[0], ck2.scale_set[1])
    ref = oracle.classify_test(ck2.layer_weights, ck2.layer_bias, x)[0]
    assert np.abs(m.classify_test(x)[0] - ref).max() <= 2e-6
    srt = np.sort(ref)
    if srt[-1] - srt[-2] > 1e-4:
        assert m.classify_file(f) == oracle.classify_argmax(ref)              # RCN::classify incl. PNG decode == oracle


def test_cpp_cli_binary_matches_reference_flow(tmp_path):
    """mercer_research_amd/rcn_hip_cli (C++, = rcn/src/main.rs over the C ABI): PNG directories in, epoch lines out,
    rcn.bin written in the reference's bincode format and readable by the Python codec; a second run resumes."""
    import subprocess
    from mercer_research_amd import build as hb, checkpoint
    exe = hb.build_cli()
    rng = np.random.default_rng(4)
    protos = []
    for _ in range(10):
        p = np.zeros((28, 28), dtype=np.uint8)
        p[4:24, 4:24] = np.where(rng.random((20, 20)) < 0.3, rng.integers(80, 256, (20, 20)), 0)
        protos.append(p)
    tr, te, model_path = str(tmp_path / "training"), str(tmp_path / "testing"), str(tmp_path / "rcn.bin")
    _write_png_set(tr, protos, 30, rng)
    _write_png_set(te, protos, 10, rng)
    argv = [exe, "--training-path", tr, "--testing-path", te, "--training-class-size", "30", "--testing-class-size", "10", "-b", "10", "-e", "4",
            "--model-path", model_path, "--seed", "9"]
    out = subprocess.run(argv, capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stdout + out.stderr
    lines = out.stdout.strip().splitlines()
    assert len(lines) == 4 and all(l.startswith(f"Epoch {i}: ") and "/100 [" in l and l.endswith("%]") for i, l in enumerate(lines))
    acc = [int(l.split(": ")[1].split("/")[0]) for l in lines]
    ck = checkpoint.loads(open(model_path, "rb").read())
    assert ck.classes == 10 and [w.shape for w in ck.layer_weights] == [(30, 784), (10, 30)] and ck.testing_path == te

    # Properties instead of "this seed trains" (VERDICT r2): (1) the count the last epoch line prints IS the accuracy of the model the
    # run saved -- recomputed here by an independent route: the Python codec reads rcn.bin, the Python PNG decoder reads every test
    # file, RCN::classify's arg-max (rcn.rs:82-98) against the class directory's index; the epoch line counts `v == max` one-hot
    # matches (rcn.rs:152-157), which differs from the arg-max only on exact ties of the output layer, so files with a runner-up
    # closer than 1e-5 are set aside;
    def saved_model_accuracy(path):
        m = checkpoint.load_model(path)
        hits = unsure = 0
        for ci, cdir in enumerate(sorted(os.listdir(te))):
            for f in sorted(os.listdir(os.path.join(te, cdir))):
                img = _png.to_pixel_matrix_u8(open(os.path.join(te, cdir, f), "rb").read())
                out_v = m.classify_test(m.standardize(m.flatten_feature_set(img[None])))[0]
                srt = np.sort(out_v)
                unsure += int(srt[-1] - srt[-2] <= 1e-5)
                hits += int(int(np.flatnonzero(out_v == out_v.max())[-1]) == ci)
        m.close()
        return hits, unsure
    from mercer_research_amd import png as _png
    hits, unsure = saved_model_accuracy(model_path)
    assert abs(acc[-1] - hits) <= unsure, (acc, hits, unsure)
    # (2) a seeded run is reproducible: the same command prints the same four lines and writes the same bytes;
    model_b = str(tmp_path / "rcn_b.bin")
    again = subprocess.run(argv[:-4] + ["--model-path", model_b, "--seed", "9"], capture_output=True, text=True, timeout=300)
    assert again.returncode == 0 and again.stdout == out.stdout
    ckb = checkpoint.loads(open(model_b, "rb").read())
    assert all(np.array_equal(x, y) for x, y in zip(ckb.layer_weights + ckb.layer_bias, ck.layer_weights + ck.layer_bias))
    # (3) a second run RESUMES: it starts from the saved weights (its one epoch line equals the accuracy of the model IT saves, and a
    # run of zero further steps would have printed acc[-1]); training one more epoch from there does not fall back to chance (10/100)
    out2 = subprocess.run(argv[:-6] + ["-e", "1", "--model-path", model_path, "--seed", "10"], capture_output=True, text=True, timeout=300)
    assert out2.returncode == 0
    acc2 = int(out2.stdout.split(": ")[1].split("/")[0])
    hits2, unsure2 = saved_model_accuracy(model_path)
    assert abs(acc2 - hits2) <= unsure2, (acc2, hits2, unsure2)
    ck3 = checkpoint.loads(open(model_path, "rb").read())
    assert not np.array_equal(ck3.layer_weights[0], ck.layer_weights[0])                   # it trained on ...
    assert float(np.abs(ck3.layer_weights[0] - ck.layer_weights[0]).mean()) < 0.25 * float(np.abs(ck.layer_weights[0]).mean())   # ... from the saved weights, not from a fresh N(0,1) draw
    bad = subprocess.run(argv[:5] + ["--training-class-size", "31", "--testing-class-size", "10", "--model-path", str(tmp_path / "x.bin")],
                         capture_output=True, text=True, timeout=300)
    assert bad.returncode == 101 and "too large! expected 31 <= 30" in bad.stderr       # rcn.rs:383-390 panic
