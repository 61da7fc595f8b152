"""The sample group's half of the resident one-XCD kernel's step in the single-GPU f32 forms for 64 samples and more: the cost share
only where somebody reads it, the image words in the order of their first use through one address register (csrc/dense_xcd.hpp:
kTailCost, kTailWordsByUse).  The cases were chosen for the whole of that half as it was tried -- wave 0 summing the slab in registers,
the two delta_1 chains as one region (profiles/resident_tail_dropped_*.patch) -- and hold whatever is put there next.  The results
must be what they were.

Bit equality, new code against old.  The data-parallel form keeps the old sample-group code, and at a group of ONE rank its exchange
adds nothing: the gathered sum is the rank's own partial.  So the single-GPU form must give the data-parallel form's parameters and
per-step costs as bits (set up as tests/test_gpu_resident_step_top.py: bootstrap over RCCL forced on).

The slab sum adds producer p into accumulator p % 8 (wave p % 8 today), so the inputs are chosen for the producer count NA = ceil(ceil(F / 16) / 2):
    F =  36 -> NA =  2   accumulators 2..7 stay empty, no whole group of four
    F = 256 -> NA =  8   every accumulator once          F = 288 -> NA =  9   the first wrap of p % 8
    F = 512 -> NA = 16                                    F = 544 -> NA = 17
    F = 784 -> NA = 25   the bench's net                  F = 928 -> NA = 29   the largest (29 + 3 tail tiles = 32 workers)
Batches 64, 128 and 256;
1, 2, 3 and 5 steps; a shuffled index, the same index entered one batch in, and no index.  Hidden sizes 16, 17, 30 and 32 at F = 36:
the second hidden tile of delta_1 is all padding, one unit, masked, then full.  Classes 10 and 16.

Cost on and off: the same calls with a cost buffer and with None give the same parameters as bits; the costs, where asked for, are
finite, positive and the twin's bits.

Oracle tolerance where no twin exists: the padded batches 100 and 200, the two-hidden-layer net 784-10-10-10 at 256 and 100 samples
and the gather form at 256 -- one step and six chained steps at the tolerances of tests/test_gpu_round3.py, two runs equal as bits.

Every case asserts that the resident kernel is what answers and that nothing stepped down.  Nothing here sets a fault option.
"""
import numpy as np
import pytest

from oracle.rcn_oracle import one_hot, synthetic_params

pytestmark = pytest.mark.gpu

ROWS = 5 * 256


def _net(shape, convpool, F, hidden=30, classes=10):
    return dict(input_shape=shape, convpool=convpool, F=F, NA=-(-(-(-F // 16)) // 2), hidden=hidden, classes=classes)


# one convolve + pool pair gives (h / 2) (w / 2) 4 features, the default two pairs (h / 4) (w / 4) 16
NETS = {"36-30-10": _net((6, 6), "one", 36), "256-30-10": _net((16, 16), "one", 256), "288-30-10": _net((16, 18), "one", 288),
        "512-30-10": _net((16, 32), "one", 512), "544-30-10": _net((16, 34), "one", 544), "784-30-10": _net((28, 28), "default", 784),
        "928-30-10": _net((16, 58), "one", 928),
        "36-16-10": _net((6, 6), "one", 36, hidden=16), "36-17-10": _net((6, 6), "one", 36, hidden=17),
        "36-32-10": _net((6, 6), "one", 36, hidden=32), "36-30-16": _net((6, 6), "one", 36, classes=16),
        "784-30-16": _net((28, 28), "default", 784, classes=16)}
WANT_NA = {"36-30-10": 2, "256-30-10": 8, "288-30-10": 9, "512-30-10": 16, "544-30-10": 17, "784-30-10": 25, "928-30-10": 29}
BATCHES = (64, 128, 256)
FORMS = (("shuffled", (1, 2, 3, 5)), ("offset", (4,)), ("stored", (1, 2, 3, 5)))
TWIN_CASES = [(net, B, form, nb) for net in NETS for B in BATCHES for form, nbs in FORMS for nb in nbs]
COST_CASES = [(net, B) for net in ("36-30-10", "288-30-10", "784-30-10", "928-30-10", "36-17-10", "36-30-16") for B in BATCHES]

# tests/test_gpu_round3.py, the resident kernel against the reference loop (f32): one step from identical parameters,
# and six chained steps in a shuffled order -- (relative, absolute) of a parameter, relative of a cost
ONE_STEP = (1e-5, 1e-6, 1e-5)
SIX_STEPS = (1e-4, 1e-5, 1e-4)


def test_the_nets_cover_the_producer_counts():
    for net, na in WANT_NA.items():
        assert NETS[net]["NA"] == na, (net, NETS[net]["NA"])


class _Twin:
    """one net: its data on the device, a single-GPU context (new sample-group code) and a data-parallel context at a group of one (old)"""

    def __init__(self, net):
        import mercer_research_amd as amd
        from mercer_research_amd.device import DeviceRCN
        spec = NETS[net]
        L = amd.RCNLayer
        convpool = None if spec["convpool"] == "default" else [L.Convolve2D(amd.Padding.SAME), L.Pool2D(amd.Pooling.MAX)]
        F, H, C = spec["F"], spec["hidden"], spec["classes"]
        rng = np.random.default_rng(52000 + F + 7 * H + C)
        X = np.maximum(rng.standard_normal((ROWS, F)), 0.0).astype(np.float32)
        Y = np.eye(C, dtype=np.float32)[rng.integers(0, C, ROWS)]
        perm = rng.permutation(ROWS).astype(np.int32)
        ws, bs = synthetic_params([F, H, C], seed=42)
        self.ws, self.bs = [w * 0.1 for w in ws], bs
        self.ctx = {}
        for form in ("single", "dp"):
            d = DeviceRCN(classes=C, convpool_cfg=convpool, feedforward_cfg=[H], input_shape=spec["input_shape"], dtype=amd.F32)
            assert d.F == F
            assert -(-(-(-d.F // 16)) // 2) == spec["NA"], "the producer count this net is here for"
            d.set_dense_path(5)                          # the resident kernel or an error: no other path can answer
            if form == "dp":
                try:
                    assert d.dp_init() == (0, 1)
                except amd.RcnHipError as e:
                    pytest.skip(f"no RCCL bootstrap on this box: {e}")
                assert d.dp_p2p_mode() == 2
            self.ctx[form] = (d, d.to_device(X), d.to_device(Y), d.to_device(perm))

    def run(self, which, B, form, nb, cost=True):
        """-> (parameters, per-step costs or None) of one call of nb steps from the starting parameters"""
        d, X, Y, perm = self.ctx[which]
        assert d.train_epoch_resident(B)
        if which == "dp":
            assert d.dp_resident(B)
        d.set_params(self.ws, self.bs)
        loss = d.empty(nb) if cost else None
        index = {"shuffled": perm, "offset": perm[B:], "stored": None}[form]
        (d.dp_train_epoch if which == "dp" else d.train_epoch)(X, Y, index, B, nb, 3.0, loss)
        d.synchronize()
        assert d.fallbacks_taken() == 0, "a launch stepped down to another path"
        return d.params_flat().cpu().numpy().copy(), (loss.cpu().numpy().copy() if cost else None)

    def close(self):
        if "dp" in self.ctx:
            self.ctx["dp"][0].dp_finalize()
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
def test_new_sample_group_computes_the_old_one_s_bits(twins, net, B, form, nb):
    twin = twins(net)
    want_p, want_c = twin.run("dp", B, form, nb)
    got_p, got_c = twin.run("single", B, form, nb)
    print(net, "NA", NETS[net]["NA"], B, form, nb, "costs", got_c.tolist())
    assert np.all(np.isfinite(want_c)) and want_c.min() > 0.0, "the old code's costs are not those of a training step"
    assert np.array_equal(got_c.view(np.uint32), want_c.view(np.uint32)), f"per-step costs differ: {got_c - want_c}"
    assert np.array_equal(got_p.view(np.uint32), want_p.view(np.uint32)), f"parameters differ at {np.flatnonzero(got_p != want_p)[:8]}"


@pytest.mark.parametrize("net,B", COST_CASES, ids=[f"{n}-B{b}" for n, b in COST_CASES])
def test_parameters_do_not_depend_on_whether_a_cost_is_asked_for(twins, net, B):
    twin = twins(net)
    for form, nb in (("shuffled", 3), ("stored", 1)):
        want_p, want_c = twin.run("dp", B, form, nb)
        with_p, with_c = twin.run("single", B, form, nb, cost=True)
        none_p, _ = twin.run("single", B, form, nb, cost=False)
        again_p, again_c = twin.run("single", B, form, nb, cost=True)          # (a cost again behind a call without one)
        print(net, B, form, nb, "costs", with_c.tolist())
        assert np.all(np.isfinite(with_c)) and with_c.min() > 0.0
        assert np.array_equal(with_c.view(np.uint32), want_c.view(np.uint32)), f"costs differ from the twin's: {with_c - want_c}"
        assert np.array_equal(again_c.view(np.uint32), want_c.view(np.uint32)), f"costs differ from the twin's: {again_c - want_c}"
        assert np.array_equal(none_p.view(np.uint32), with_p.view(np.uint32)), f"parameters differ at {np.flatnonzero(none_p != with_p)[:8]}"
        assert np.array_equal(again_p.view(np.uint32), with_p.view(np.uint32))
        assert np.array_equal(with_p.view(np.uint32), want_p.view(np.uint32)), f"parameters differ at {np.flatnonzero(with_p != want_p)[:8]}"


ORACLE_CASES = [("784-30-10", [30], 100, 0), ("784-30-10", [30], 200, 0), ("784-10-10-10", [10, 10], 256, 0), ("784-10-10-10", [10, 10], 100, 0),
                ("784-30-10-gather", [30], 256, 1)]


def _close(got, want, tol, what):
    rel, ab, _ = tol
    for a, b in zip(got, want):
        err = np.abs(a - b) - (rel * np.abs(b) + ab)
        print(what, "largest |d| =", float(np.abs(a - b).max()), "over the bound by", float(err.max()))
        assert np.all(err <= 0.0), (what, float(np.abs(a - b).max()))


@pytest.mark.parametrize("name,hidden,B,gather", ORACLE_CASES, ids=[f"{n}-B{b}" for n, _, b, _ in ORACLE_CASES])
def test_forms_without_a_twin_are_the_reference_loop(oracle, name, hidden, B, gather):
    from mercer_research_amd.device import DeviceRCN
    dims = [784] + hidden + [10]
    N, nb = 2048, 6
    rng = np.random.default_rng(5200 + B + len(hidden))
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
    # the same seven steps without a cost buffer: the same parameters as bits
    d.set_params(ws, bs)
    d.train_epoch(Xd, Yd, None, B, 1, 3.0, None)
    d.train_epoch(Xd, Yd, pd, B, nb, 3.0, None)
    d.synchronize()
    assert d.fallbacks_taken() == 0, "a launch stepped down to another path"
    costless = d.params_flat().cpu().numpy().copy()
    d.rcn.close()
    # two runs of the same calls: the same bits
    assert np.array_equal(runs[0][2].view(np.uint32), runs[1][2].view(np.uint32)), runs[0][2] - runs[1][2]
    assert np.array_equal(runs[0][3].view(np.uint32), runs[1][3].view(np.uint32))
    assert np.array_equal(runs[0][3].view(np.uint32), costless.view(np.uint32)), "the parameters depend on whether a cost was asked for"
    for a, b in zip(runs[0][0], runs[1][0]):
        assert np.array_equal(np.asarray(a), np.asarray(b))
    p1, p7, costs, _ = runs[0]
    costs = costs.astype(np.float64)
    assert np.all(np.isfinite(costs)) and costs.min() > 0.0
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
