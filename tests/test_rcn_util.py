"""The shared checks of tests/_rcn_util.py still bite, and its data draw is the one the pair files made themselves (CPU, no device)."""
import re
from fractions import Fraction

import numpy as np
import pytest
from _rcn_util import (F32, F32_ONE_STEP, F32_SIX_STEPS, F64, F64_ONE_STEP, F64_SIX_STEPS, FEATURE_NETS, close_to, draw_rows, feature_net, index_of,
                       one_and_six_inputs, same_bits)

BITS = {np.float32: np.uint32, np.float64: np.uint64}


def _flip_low_bit(a, i, bits):
    out = a.copy()
    out.view(bits)[i] ^= 1
    return out


@pytest.mark.parametrize("np_t", [np.float32, np.float64], ids=["f32", "f64"])
def test_same_bits_passes_on_equal_arrays_and_raises_on_every_kind_of_difference(np_t):
    bits = BITS[np_t]
    rng = np.random.default_rng(7)
    p, c = rng.standard_normal(50).astype(np_t), (rng.random(5) + 0.5).astype(np_t)
    p[3] = 0.0
    same_bits((p.copy(), c.copy()), (p, c), bits, "equal")
    same_bits((p.copy(), None), (p, c), bits, "a call without costs, equal parameters")
    minus_zero = p.copy()
    minus_zero[3] = -0.0
    assert np.array_equal(minus_zero, p)                             # ... which a comparison of values lets through
    nan_cost, zero_cost = c.copy(), c.copy()
    nan_cost[2], zero_cost[2] = np.nan, 0.0
    for what, got, want in (("one flipped low bit in a parameter", (_flip_low_bit(p, 17, bits), c), (p, c)),
                            ("one flipped low bit in a parameter of a call without costs", (_flip_low_bit(p, 17, bits), None), (p, c)),
                            ("one flipped low bit in a cost", (p, _flip_low_bit(c, 4, bits)), (p, c)),
                            ("+0.0 against -0.0", (minus_zero, c), (p, c)),
                            ("a NaN cost on both sides", (p, nan_cost), (p, nan_cost)),
                            ("a NaN cost", (p, nan_cost), (p, c)),
                            ("a zero cost on both sides", (p, zero_cost), (p, zero_cost)),
                            ("a zero cost", (p, c), (p, zero_cost))):
        with pytest.raises(AssertionError, match=re.escape(what)):
            same_bits(got, want, bits, what)


@pytest.mark.parametrize("tol", [F32_ONE_STEP, F32_SIX_STEPS, F64_ONE_STEP, F64_SIX_STEPS], ids=["f32-one-step", "f32-six-steps", "f64-one-step", "f64-six-steps"])
def test_close_to_passes_at_the_bound_and_raises_one_ulp_above_it(tol):
    rel, ab, _ = tol
    # want = 0: the bound is `ab` itself, and got = ab is exactly on it
    want = [np.zeros(3)]
    close_to([np.array([0.0, ab, -ab])], want, tol, "on the absolute bound")
    for over in (np.nextafter(ab, 1.0), -np.nextafter(ab, 1.0)):
        with pytest.raises(AssertionError):
            close_to([np.array([0.0, ab, over])], want, tol, "one ulp above the absolute bound")
    # want = 1: got = 1 + k * 2^-52 differs from it by exactly k * 2^-52 -- k the last one within rel * 1 + ab, then the next one
    bound, ulp = rel * 1.0 + ab, 2.0 ** -52
    k = int(Fraction(bound) // Fraction(ulp))
    assert Fraction(k) * Fraction(ulp) <= Fraction(bound) < Fraction(k + 1) * Fraction(ulp)
    want = [np.zeros(2), np.ones(2)]
    close_to([np.zeros(2), np.array([1.0, 1.0 + k * ulp])], want, tol, "the last value within the bound")
    with pytest.raises(AssertionError):
        close_to([np.zeros(2), np.array([1.0, 1.0 + (k + 1) * ulp])], want, tol, "one ulp above the bound")


def test_the_tolerances_are_the_ones_the_files_held():
    assert (F32_ONE_STEP, F32_SIX_STEPS) == ((1e-5, 1e-6, 1e-5), (1e-4, 1e-5, 1e-4))
    assert (F64_ONE_STEP, F64_SIX_STEPS) == ((1e-11, 1e-12, 1e-11), (1e-10, 1e-11, 1e-10))


# (file, spec, dtype, B) and, written out as the file wrote them, the rows and the seed of its draw
POLICIES = [("test_gpu_resident_step_top.py", FEATURE_NETS["784-30-10"], F32, 64, 5 * 256, 31000 + 784),
            ("test_gpu_resident_tail.py", feature_net((6, 6), "one", 36, hidden=17, classes=16), F32, 128, 5 * 256, 52000 + 36 + 7 * 17 + 16),
            ("test_gpu_resident_prefetch.py", FEATURE_NETS["36-30-10"], F32, 256, 5 * 256, 20250 + 36),
            ("test_gpu_pack_forms.py", FEATURE_NETS["784-30-10"], F64, 100, 5 * 100, 20250 + 784 + 100)]


@pytest.mark.parametrize("spec,dtype,B,rows,seed", [p[1:] for p in POLICIES], ids=[p[0] for p in POLICIES])
def test_the_pairs_draw_is_the_draw_the_file_made_itself(spec, dtype, B, rows, seed):
    np_t = np.float64 if dtype == F64 else np.float32
    rng = np.random.default_rng(seed)                                # the file's own lines: X, then Y, then perm, from one generator
    X = np.maximum(rng.standard_normal((rows, spec["F"])), 0.0).astype(np_t)
    Y = np.eye(spec["classes"], dtype=np_t)[rng.integers(0, spec["classes"], rows)]
    perm = rng.permutation(rows).astype(np.int32)
    gX, gY, gperm = draw_rows(spec, dtype, rows, seed)
    assert gX.dtype == X.dtype and gX.shape == X.shape and np.array_equal(gX[0], X[0]) and X[0].max() > 0.0
    assert gperm.dtype == np.int32 and np.array_equal(gperm[:B], perm[:B]) and np.array_equal(np.sort(gperm), np.arange(rows))
    assert gY.dtype == Y.dtype and np.array_equal(gY, Y)
    assert index_of(gperm, B, "shuffled") is gperm and np.array_equal(index_of(gperm, B, "offset"), perm[B:]) and index_of(gperm, B, "stored") is None


def test_the_oracle_tests_draw_and_both_parameter_generators():
    """one_and_six_inputs against the lines of tests/test_gpu_round3.py (seed 100 + B, through f32) and tests/test_gpu_round4.py (300 + B,
    f64); and synthetic_params of mercer_research_amd.synth, which two of the pair files used, is the oracle's, which the helper uses"""
    from mercer_research_amd.synth import synthetic_params as synth_params
    from oracle.rcn_oracle import one_hot, synthetic_params
    for seed, dtype, hidden in ((100 + 33, F32, [30]), (300 + 255, F64, [10, 10])):
        rng = np.random.default_rng(seed)
        X = np.maximum(rng.standard_normal((2048, 784)), 0.0)
        if dtype == F32:
            X = X.astype(np.float32).astype(np.float64)
        Y = one_hot(rng.integers(0, 10, 2048))
        ws, bs = synthetic_params([784] + hidden + [10], seed=21)
        perm = rng.permutation(2048).astype(np.int32)
        gX, gY, gperm, gws, gbs = one_and_six_inputs(hidden, seed, dtype)
        assert gX.dtype == np.float64 and np.array_equal(gX, X) and np.array_equal(gY, Y) and np.array_equal(gperm, perm)
        assert all(np.array_equal(a, b * 0.1) for a, b in zip(gws, ws)) and all(np.array_equal(a, b) for a, b in zip(gbs, bs))
    for dims in ([784, 30, 10], [36, 30, 10], [100, 30, 10]):
        for a, b in zip(sum(synth_params(dims, seed=42), []), sum(synthetic_params(dims, seed=42), [])):
            assert a.dtype == b.dtype and np.array_equal(a, b), dims
