"""The step top of the resident one-XCD kernel's single-GPU f32 forms for 64 samples and more: ONE wait for the slab and the tail flags,
the image words fetched behind the step-top barrier, the first loads of a phase issued in front of the look at the abort word
(csrc/dense_xcd.hpp: kOneTopWait, kMfmaFirst).  The results must be what they were.

Bit equality, new top against old top.  The data-parallel form keeps the old step top, and at a group of ONE rank its exchange adds
nothing: the gathered sum is the rank's own partial.  So the single-GPU form must give the data-parallel form's parameters and
per-step costs as bits (set up as tests/test_gpu_round2.py's test of the two forms at world one: bootstrap over RCCL forced on).
Nets 784-30-10 (the last feature worker holds ONE slice) and 36-30-10 (three slices: worker 1 has no second one); batches 64, 128 and
256, the shard sizes the data-parallel form exists for among the tiles of 64 samples and more; 1, 2, 3 and 5 steps -- the prologue
alone, the first look-ahead, and the last steps whose fetches are suppressed; a shuffled index, the same index entered one batch in,
and no index.

Oracle tolerance where no old-top twin exists: the padded batches 100 and 200 (the forms with the batch length a run-time value),
the two-hidden-layer net 784-10-10-10 at 256 and 100 samples, and the gather form at 256.  One step and six chained steps at the
tolerances of tests/test_gpu_round3.py (test_resident_kernel_at_any_batch_of_1_to_256_is_the_reference_loop), and two runs of the
same calls equal as bits.

Every case asserts that the resident kernel is what answers and that nothing stepped down.  Nothing here sets a fault option: the
time-out record of the merged wait is held by the static_asserts beside xcd_top_missing.
"""
import numpy as np
import pytest

from oracle.rcn_oracle import one_hot, synthetic_params

pytestmark = pytest.mark.gpu

ROWS = 5 * 256
NETS = {"784-30-10": dict(input_shape=(28, 28), convpool="default", F=784),
        "36-30-10": dict(input_shape=(6, 6), convpool="one", F=36)}
BATCHES = (64, 128, 256)
FORMS = (("shuffled", (1, 2, 3, 5)), ("offset", (4,)), ("stored", (1, 2, 3, 5)))
TWIN_CASES = [(net, B, form, nb) for net in NETS for B in BATCHES for form, nbs in FORMS for nb in nbs]

# tests/test_gpu_round3.py, the resident kernel against the reference loop (f32): one step from identical parameters,
# and six chained steps in a shuffled order -- (relative, absolute) of a parameter, relative of a cost
ONE_STEP = (1e-5, 1e-6, 1e-5)
SIX_STEPS = (1e-4, 1e-5, 1e-4)


class _Twin:
    """one net: its data on the device, a single-GPU context (new step top) and a data-parallel context at a group of one (old)"""

    def __init__(self, net):
        import mercer_research_amd as amd
        from mercer_research_amd.device import DeviceRCN
        spec = NETS[net]
        L = amd.RCNLayer
        convpool = None if spec["convpool"] == "default" else [L.Convolve2D(amd.Padding.SAME), L.Pool2D(amd.Pooling.MAX)]
        rng = np.random.default_rng(31000 + spec["F"])
        X = np.maximum(rng.standard_normal((ROWS, spec["F"])), 0.0).astype(np.float32)
        Y = np.eye(10, dtype=np.float32)[rng.integers(0, 10, ROWS)]
        perm = rng.permutation(ROWS).astype(np.int32)
        ws, bs = synthetic_params([spec["F"], 30, 10], seed=42)
        self.ws, self.bs = [w * 0.1 for w in ws], bs
        self.ctx = {}
        for form in ("single", "dp"):
            d = DeviceRCN(classes=10, convpool_cfg=convpool, feedforward_cfg=[30], input_shape=spec["input_shape"], dtype=amd.F32)
            assert d.F == spec["F"]
            d.set_dense_path(5)                          # the resident kernel or an error: no other path can answer
            if form == "dp":
                try:
                    assert d.dp_init() == (0, 1)
                except amd.RcnHipError as e:
                    pytest.skip(f"no RCCL bootstrap on this box: {e}")
                assert d.dp_p2p_mode() == 2
            self.ctx[form] = (d, d.to_device(X), d.to_device(Y), d.to_device(perm))

    def run(self, which, B, form, nb):
        """-> (parameters, per-step costs) of one call of nb steps from the starting parameters"""
        d, X, Y, perm = self.ctx[which]
        assert d.train_epoch_resident(B)
        if which == "dp":
            assert d.dp_resident(B)
        d.set_params(self.ws, self.bs)
        loss = d.empty(nb)
        index = {"shuffled": perm, "offset": perm[B:], "stored": None}[form]
        (d.dp_train_epoch if which == "dp" else d.train_epoch)(X, Y, index, B, nb, 3.0, loss)
        d.synchronize()
        assert d.fallbacks_taken() == 0, "a launch stepped down to another path"
        return d.params_flat().cpu().numpy().copy(), loss.cpu().numpy().copy()

    def close(self):
        d = self.ctx["dp"][0]
        d.dp_finalize()
        for d, *_ in self.ctx.values():
            d.rcn.close()


@pytest.fixture(scope="module")
def twins():
    made = {}
    with pytest.MonkeyPatch.context() as mp:
        mp.setenv("RCN_HIP_DP_P2P", "2")

        def get(net):
            if net not in made:
                made[net] = _Twin(net)
            return made[net]

        yield get
        for t in made.values():
            t.close()


@pytest.mark.parametrize("net,B,form,nb", TWIN_CASES, ids=[f"{n}-B{b}-{f}-{k}steps" for n, b, f, k in TWIN_CASES])
def test_new_step_top_computes_the_old_step_top_s_bits(twins, net, B, form, nb):
    twin = twins(net)
    want_p, want_c = twin.run("dp", B, form, nb)
    got_p, got_c = twin.run("single", B, form, nb)
    print(net, B, form, nb, "costs", got_c.tolist())
    assert np.all(np.isfinite(want_c)) and want_c.min() > 0.0, "the old step top's costs are not those of a training step"
    assert np.array_equal(got_c.view(np.uint32), want_c.view(np.uint32)), f"per-step costs differ: {got_c - want_c}"
    assert np.array_equal(got_p.view(np.uint32), want_p.view(np.uint32)), f"parameters differ at {np.flatnonzero(got_p != want_p)[:8]}"


ORACLE_CASES = [("784-30-10", [30], 100, 0), ("784-30-10", [30], 200, 0), ("784-10-10-10", [10, 10], 256, 0), ("784-10-10-10", [10, 10], 100, 0),
                ("784-30-10-gather", [30], 256, 1)]


def _close(got, want, tol, what):
    rel, ab, _ = tol
    for a, b in zip(got, want):
        err = np.abs(a - b) - (rel * np.abs(b) + ab)
        print(what, "largest |d| =", float(np.abs(a - b).max()), "over the bound by", float(err.max()))
        assert np.all(err <= 0.0), (what, float(np.abs(a - b).max()))


@pytest.mark.parametrize("name,hidden,B,gather", ORACLE_CASES, ids=[f"{n}-B{b}" for n, _, b, _ in ORACLE_CASES])
def test_forms_without_an_old_top_twin_are_the_reference_loop(oracle, name, hidden, B, gather):
    from mercer_research_amd.device import DeviceRCN
    dims = [784] + hidden + [10]
    N, nb = 2048, 6
    rng = np.random.default_rng(4100 + B + len(hidden))
    X = np.maximum(rng.standard_normal((N, 784)), 0.0).astype(np.float32).astype(np.float64)
    Y = one_hot(rng.integers(0, 10, N))
    ws, bs = synthetic_params(dims, seed=21)
    ws = [w * 0.1 for w in ws]
    perm = rng.permutation(N).astype(np.int32)
    d = DeviceRCN(dtype=0, feedforward_cfg=hidden)
    d.set_dense_path(5)                                  # the resident kernel or an error: no other path can answer
    d.set_option("xcd_gather", gather)
    assert d.train_epoch_resident(B) and d.train_epoch_gathers(B) == bool(gather)
    Xd, Yd, pd = d.to_device(X, d.tdtype), d.to_device(Y, d.tdtype), d.to_device(perm)
    runs = []
    for _ in range(2):
        d.set_params(ws, bs)
        loss = d.empty(nb + 1)
        d.train_epoch(Xd, Yd, None, B, 1, 3.0, loss)                   # one step, stored order
        p1 = sum(d.get_params(), [])
        d.train_epoch(Xd, Yd, pd, B, nb, 3.0, loss[1:])                 # six more, shuffled
        d.synchronize()
        assert d.fallbacks_taken() == 0, "a launch stepped down to another path"
        runs.append((p1, sum(d.get_params(), []), loss.cpu().numpy().copy(), d.params_flat().cpu().numpy().copy()))
    d.rcn.close()
    # two runs of the same calls: the same bits
    assert np.array_equal(runs[0][2].view(np.uint32), runs[1][2].view(np.uint32)), runs[0][2] - runs[1][2]
    assert np.array_equal(runs[0][3].view(np.uint32), runs[1][3].view(np.uint32))
    for a, b in zip(runs[0][0], runs[1][0]):
        assert np.array_equal(np.asarray(a), np.asarray(b))
    p1, p7, costs, _ = runs[0]
    costs = costs.astype(np.float64)
    rw, rb, c0 = oracle.train_batch(ws, bs, X[:B], Y[:B], 3.0)
    _close(p1, rw + rb, ONE_STEP, "one step")
    print("cost of step 0:", costs[0], "oracle", c0)
    assert abs(costs[0] - c0) <= ONE_STEP[2] * c0
    cs = []
    for j in range(nb):
        sel = perm[j * B:(j + 1) * B]
        rw, rb, c = oracle.train_batch(rw, rb, X[sel], Y[sel], 3.0)
        cs.append(c)
    print("costs of the six steps:", costs[1:].tolist(), "oracle", cs)
    np.testing.assert_allclose(costs[1:], np.array(cs), rtol=SIX_STEPS[2])
    _close(p7, rw + rb, SIX_STEPS, "six chained steps")
