"""The gather form of the resident one-XCD kernel (option "xcd_gather" = 1: the workers fetch every batch's rows themselves, by row
index, a few steps ahead) computes the same BITS as the form on the packed image (xcd_gather = 0): parameters and per-step costs, the
form chosen by the option in one process.

B = 256, the only shape the gather form exists for.  nb in {1, 2, 3, 5}: the prologue's batches alone, the first look-ahead of the
row indices, and the last three steps, whose fetches (rows two steps ahead, indices three steps ahead) must be suppressed -- a fetch
that is not would read past the 5 x 256 index words and rows these calls own.  Three index forms: a shuffled index, the same index
entered one batch in (perm[B:], four steps), and no index (stored order).  Two nets: 784-30-10, whose last feature worker holds ONE
16-feature slice, and 36-30-10 -- three slices, so worker 1 has a first slice and no second one.

Equality, not a tolerance: the two forms load the same words and run the same arithmetic in the same order.  Nothing here sets a
fault option.
"""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

B = 256
ROWS = 5 * B
NETS = {"784-30-10": dict(input_shape=(28, 28), convpool="default", F=784),
        "36-30-10": dict(input_shape=(6, 6), convpool="one", F=36)}
CASES = [(net, form, nb) for net in NETS for form, nbs in (("shuffled", (1, 2, 3, 5)), ("offset", (4,)), ("stored", (1, 2, 3, 5))) for nb in nbs]


class _Pair:
    """one net: its data on the device, and a context per form"""

    def __init__(self, net):
        import torch
        import mercer_research_amd as amd
        from mercer_research_amd.device import DeviceRCN
        from mercer_research_amd.synth import synthetic_params
        spec = NETS[net]
        L = amd.RCNLayer
        convpool = None if spec["convpool"] == "default" else [L.Convolve2D(amd.Padding.SAME), L.Pool2D(amd.Pooling.MAX)]
        rng = np.random.default_rng(20250 + spec["F"])
        self.X_h = np.maximum(rng.standard_normal((ROWS, spec["F"])), 0.0).astype(np.float32)
        self.Y_h = np.eye(10, dtype=np.float32)[rng.integers(0, 10, ROWS)]
        self.perm_h = rng.permutation(ROWS).astype(np.int32)
        ws, bs = synthetic_params([spec["F"], 30, 10], seed=42)
        self.ws, self.bs = [w * 0.1 for w in ws], bs
        self.ctx = {}
        for form, opt in (("packed", 0), ("gather", 1)):
            d = DeviceRCN(classes=10, convpool_cfg=convpool, feedforward_cfg=[30], input_shape=spec["input_shape"], dtype=amd.F32)
            assert d.F == spec["F"]
            d.set_dense_path(5)                          # the resident kernel or an error: no other path can answer
            d.set_option("xcd_gather", opt)
            assert d.train_epoch_resident(B)
            assert d.train_epoch_gathers(B) == bool(opt)
            self.ctx[form] = (d, d.to_device(self.X_h), d.to_device(self.Y_h), d.to_device(self.perm_h))

    def run(self, which, form, nb):
        """-> (parameters, per-step costs) of one call of nb steps from the starting parameters"""
        d, X, Y, perm = self.ctx[which]
        d.set_params(self.ws, self.bs)
        loss = d.empty(nb)
        index = {"shuffled": perm, "offset": perm[B:], "stored": None}[form]
        d.train_epoch(X, Y, index, B, nb, 3.0, loss)
        d.synchronize()
        assert d.fallbacks_taken() == 0, "a launch stepped down to another path"
        return d.params_flat().cpu().numpy().copy(), loss.cpu().numpy().copy()

    def close(self):
        for d, *_ in self.ctx.values():
            d.rcn.close()


@pytest.fixture(scope="module")
def pairs():
    made = {}

    def get(net):
        if net not in made:
            made[net] = _Pair(net)
        return made[net]

    yield get
    for p in made.values():
        p.close()


@pytest.mark.parametrize("net,form,nb", CASES, ids=[f"{n}-{f}-{k}steps" for n, f, k in CASES])
def test_gather_form_computes_the_packed_form_s_bits(pairs, net, form, nb):
    pair = pairs(net)
    want_p, want_c = pair.run("packed", form, nb)
    got_p, got_c = pair.run("gather", form, nb)
    print(net, form, nb, "costs", got_c.tolist())
    assert np.all(np.isfinite(want_c)) and want_c.min() > 0.0, "the packed form's costs are not those of a training step"
    assert np.array_equal(got_c.view(np.uint32), want_c.view(np.uint32)), f"per-step costs differ: {got_c - want_c}"
    assert np.array_equal(got_p.view(np.uint32), want_p.view(np.uint32)), f"parameters differ at {np.flatnonzero(got_p != want_p)[:8]}"
