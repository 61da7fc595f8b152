"""The epoch image gathered by k_pack_rows (option "pack_form" = 1, the default: whole rows per workgroup, every row index loaded once
ahead of the rows, pieces moved in groups of loads then stores) is the image k_pack_epoch writes (pack_form = 0), byte for byte.

Two contexts that differ only in that option start from the same parameters and make the same call; the parameters and the per-step
costs must come out EQUAL AS BITS -- the image is the only thing that differs between them, and it must not.  Every case also holds the
costs finite and positive and that no launch stepped down to another path.  Nothing here sets a fault option.

The cases are the smallest at which the new kernel can go wrong:
  nets      784-30-10 (G = 49: rows of 24.5 lines, so odd rows start mid-line, and the last slice pair has one slice), 36-30-10 (G = 3:
            the whole row is "edge" pieces and the last slice is part zeros), 100-30-10 (G = 7: two whole steps, an edge, three pieces of
            zeros) -- each with each index form;
  rows      the scalar-row kernels (VECX = false).  No conv / pool stack the constructor takes for training gives F % 4 != 0 (a stack
            without a Convolve2D layer has no features at all, and with one F is a multiple of four), so the form is entered the other
            way the launcher enters it: a feature matrix that does not start on 16 bytes -- 784-30-10 and 36-30-10 (where elements past
            F are zeros) one float off, each with each index form;
  batches   256, 100 (rows not a multiple of a workgroup's 32; the resident kernel on a partial tile), 10, 300 (above the resident
            kernel: the two-kernel pipeline reads the image);
  indices   a shuffled index, the same index entered one batch in (perm[B:], at most four steps), none (stored order);
  steps     1, 3, and 5 with pack_segment_bytes worth two batches, so that both halves of the image are used and re-packed in the call;
  entry     epoch_begin + epoch_steps(0, 1) + epoch_steps(1, 2) against train_epoch over the same three batches;
  dtype     f32 for all of these, f64 for 784-30-10 at B = 10 and 100.
One more case does not rest on k_pack_epoch being right: pack_form = 1 against the gather form of the resident kernel (xcd_gather = 1),
which never runs a pack kernel.
"""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

NETS = {"784-30-10": dict(input_shape=(28, 28), convpool="default", F=784, path=0),
        "36-30-10": dict(input_shape=(6, 6), convpool="one", F=36, path=0),
        "100-30-10": dict(input_shape=(10, 10), convpool="one", F=100, path=0),
        "784-30-10/unaligned": dict(input_shape=(28, 28), convpool="default", F=784, path=0, unaligned=True),
        "36-30-10/unaligned": dict(input_shape=(6, 6), convpool="one", F=36, path=0, unaligned=True)}
#        net          dtype  B    index       what
CASES = [("784-30-10", "f32", 256, "shuffled", "3steps"),
         ("784-30-10", "f32", 256, "offset", "1step"),
         ("784-30-10", "f32", 256, "stored", "5steps-2seg"),
         ("784-30-10", "f32", 256, "shuffled", "begin"),
         ("784-30-10", "f32", 100, "shuffled", "3steps"),
         ("784-30-10", "f32", 100, "stored", "5steps-2seg"),
         ("784-30-10", "f32", 10, "stored", "1step"),
         ("784-30-10", "f32", 10, "shuffled", "5steps-2seg"),
         ("784-30-10", "f32", 300, "offset", "3steps"),
         ("784-30-10", "f32", 300, "shuffled", "5steps-2seg"),
         ("36-30-10", "f32", 256, "shuffled", "3steps"),
         ("36-30-10", "f32", 100, "offset", "3steps"),
         ("36-30-10", "f32", 10, "stored", "3steps"),
         ("36-30-10", "f32", 300, "shuffled", "5steps-2seg"),
         ("36-30-10", "f32", 256, "stored", "begin"),
         ("100-30-10", "f32", 256, "shuffled", "3steps"),
         ("100-30-10", "f32", 100, "offset", "1step"),
         ("100-30-10", "f32", 300, "stored", "3steps"),
         ("784-30-10/unaligned", "f32", 256, "shuffled", "3steps"),
         ("784-30-10/unaligned", "f32", 100, "offset", "1step"),
         ("784-30-10/unaligned", "f32", 300, "stored", "3steps"),
         ("36-30-10/unaligned", "f32", 256, "offset", "3steps"),
         ("36-30-10/unaligned", "f32", 300, "stored", "1step"),
         ("36-30-10/unaligned", "f32", 10, "shuffled", "5steps-2seg"),
         ("784-30-10", "f64", 10, "shuffled", "3steps"),
         ("784-30-10", "f64", 100, "stored", "3steps"),
         ("784-30-10", "f64", 100, "shuffled", "5steps-2seg")]
STEPS = {"1step": 1, "3steps": 3, "5steps-2seg": 5, "begin": 3}


def _make(net, dtype, options, path=None):
    import mercer_research_amd as amd
    from mercer_research_amd.device import DeviceRCN
    spec = NETS[net]
    L = amd.RCNLayer
    convpool = {"default": None, "one": [L.Convolve2D(amd.Padding.SAME), L.Pool2D(amd.Pooling.MAX)]}[spec["convpool"]]
    d = DeviceRCN(classes=10, convpool_cfg=convpool, feedforward_cfg=[30], input_shape=spec["input_shape"], dtype=amd.F64 if dtype == "f64" else amd.F32)
    assert d.F == spec["F"]
    path = spec["path"] if path is None else path
    if path:
        d.set_dense_path(path)
    for k, v in options.items():
        d.set_option(k, v)
    return d


class _Pair:
    """one net in one dtype: a context per pack form, and per batch size its data on the device"""

    def __init__(self, net, dtype, forms=(("parent", {"pack_form": 0}), ("rows", {"pack_form": 1})), path=None):
        from mercer_research_amd.synth import synthetic_params
        self.net, self.dtype, self.F = net, dtype, NETS[net]["F"]
        self.np_t = np.float64 if dtype == "f64" else np.float32
        self.bits = np.uint64 if dtype == "f64" else np.uint32
        ws, bs = synthetic_params([self.F, 30, 10], seed=42)
        self.ws, self.bs = [w * 0.1 for w in ws], bs
        self.ctx = {name: _make(net, dtype, opts, path) for name, opts in forms}
        for name, opts in forms:
            for k, v in opts.items():
                assert self.ctx[name].get_option(k) == v
        self.data = {}

    def on_device(self, which, B):
        if (which, B) not in self.data:
            rows = 5 * B
            rng = np.random.default_rng(20250 + self.F + B)
            X = np.maximum(rng.standard_normal((rows, self.F)), 0.0).astype(self.np_t)
            Y = np.eye(10, dtype=self.np_t)[rng.integers(0, 10, rows)]
            perm = rng.permutation(rows).astype(np.int32)
            d = self.ctx[which]
            if NETS[self.net].get("unaligned"):            # the same rows one element into a longer buffer
                flat = d.to_device(np.concatenate([np.zeros(1, self.np_t), X.ravel(), np.zeros(3, self.np_t)]))
                Xd = flat[1:1 + X.size].view(rows, self.F)
                assert Xd.data_ptr() % 16 == 4 and Xd.is_contiguous()
            else:
                Xd = d.to_device(X)
                assert Xd.data_ptr() % 16 == 0
            self.data[(which, B)] = (Xd, d.to_device(Y), d.to_device(perm))
        return self.data[(which, B)]

    def run(self, which, B, form, what):
        """-> (parameters, per-step costs) of one call (or one begun epoch) from the starting parameters"""
        d = self.ctx[which]
        X, Y, perm = self.on_device(which, B)
        nb = STEPS[what]
        index = {"shuffled": perm, "offset": perm[B:], "stored": None}[form]
        assert nb <= (4 if form == "offset" else 5)
        esz = 8 if self.dtype == "f64" else 4
        G = (self.F + 15) // 16
        d.set_option("pack_segment_bytes", 2 * G * B * 16 * esz if what == "5steps-2seg" else 64 << 20)
        d.set_params(self.ws, self.bs)
        loss = d.empty(nb)
        if what == "begin":
            d.epoch_begin(X, Y, index, B, nb)
            d.epoch_steps(0, 1, 3.0, loss)
            d.epoch_steps(1, 2, 3.0, loss[1:])
        else:
            d.train_epoch(X, Y, index, B, nb, 3.0, loss)
        d.synchronize()
        assert d.fallbacks_taken() == 0, "a launch stepped down to another path"
        return d.params_flat().cpu().numpy().copy(), loss.cpu().numpy().copy()

    def close(self):
        for d in self.ctx.values():
            d.rcn.close()


@pytest.fixture(scope="module")
def pairs():
    made = {}

    def get(net, dtype, **kw):
        key = (net, dtype, repr(sorted(kw.items())))
        if key not in made:
            made[key] = _Pair(net, dtype, **kw)
        return made[key]

    yield get
    for p in made.values():
        p.close()


def _same_bits(pair, got, want, what):
    (got_p, got_c), (want_p, want_c) = got, want
    assert np.all(np.isfinite(want_c)) and want_c.min() > 0.0, "the costs are not those of a training step"
    assert np.all(np.isfinite(got_c)) and got_c.min() > 0.0, "the costs are not those of a training step"
    assert np.array_equal(got_c.view(pair.bits), want_c.view(pair.bits)), f"{what}: per-step costs differ: {got_c - want_c}"
    assert np.array_equal(got_p.view(pair.bits), want_p.view(pair.bits)), f"{what}: parameters differ at {np.flatnonzero(got_p != want_p)[:8]}"


@pytest.mark.parametrize("net,dtype,B,form,what", CASES, ids=[f"{n}-{t}-B{b}-{f}-{w}" for n, t, b, f, w in CASES])
def test_pack_rows_writes_the_image_of_pack_epoch(pairs, net, dtype, B, form, what):
    pair = pairs(net, dtype)
    want = pair.run("parent", B, form, what)
    got = pair.run("rows", B, form, what)
    print(net, dtype, B, form, what, "resident", pair.ctx["rows"].train_epoch_resident(B), "costs", got[1].tolist())
    _same_bits(pair, got, want, "pack_form 1 against 0")
    if what == "begin":                                  # ... and the begun epoch walked in two pieces is train_epoch over the same three batches
        _same_bits(pair, got, pair.run("rows", B, form, "3steps"), "epoch_begin + epoch_steps against train_epoch")


def test_pack_rows_image_gives_the_gather_form_s_bits(pairs):
    """pack_form = 1 against the resident kernel fetching its rows itself: no pack kernel on that side, so this does not rest on k_pack_epoch"""
    B = 256
    pair = pairs("784-30-10", "f32", forms=(("rows", {"pack_form": 1, "xcd_gather": 0}), ("gather", {"pack_form": 1, "xcd_gather": 1})), path=5)
    for name, gathers in (("rows", False), ("gather", True)):
        assert pair.ctx[name].train_epoch_resident(B) and pair.ctx[name].train_epoch_gathers(B) == gathers
    want = pair.run("gather", B, "shuffled", "3steps")
    got = pair.run("rows", B, "shuffled", "3steps")
    print("costs", got[1].tolist())
    _same_bits(pair, got, want, "packed image against the gather form")
