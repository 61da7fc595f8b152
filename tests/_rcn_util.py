"""What the base-track GPU test files (tests/test_gpu_parity.py, tests/test_gpu_round*.py, tests/test_gpu_resident_*.py,
tests/test_gpu_pack_forms.py) share: the `amd` fixture, the oracle's loops, the tolerances and the two checks, the feature nets and their
contexts, "N contexts of one net, the same call, equal bits", "one step in stored order, six chained steps shuffled, against the oracle",
and the rank processes.  A new base-track test file starts from here; a helper only one file needs stays in that file.  Not a test file
and not a conftest: pytest does not rewrite `assert` here, so every assert carries its message."""
import os
import socket
import subprocess
import sys

import numpy as np
import pytest

from oracle.rcn_oracle import one_hot, synthetic_params

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F32, F64 = 0, 1
NP_T = {F32: np.float32, F64: np.float64}
BITS = {F32: np.uint32, F64: np.uint64}


@pytest.fixture(scope="module")
def amd():
    import mercer_research_amd as m
    return m


def xcd_or_skip(d):
    import mercer_research_amd as amd
    try:
        d.set_dense_path(5)
    except amd.RcnHipError as e:
        pytest.skip(f"the resident one-XCD kernel does not apply on this device: {e}")


# ---- the oracle's loops ------------------------------------------------------------------------------------------------------------------
def oracle_steps(oracle, ws, bs, X, Y, perm, B, nb, eta):
    rw, rb, costs = ws, bs, []
    for j in range(nb):
        sel = perm[j * B:(j + 1) * B]
        rw, rb, c = oracle.train_batch(rw, rb, X[sel], Y[sel], eta)
        costs.append(c)
    return rw, rb, np.array(costs)


def oracle_global_epochs(oracle, dims, Xs, Ys, Bs, nb, seed=17):
    """two epochs of train_batch on the ranks' shards concatenated into global batches -> (weights, biases, the first epoch's costs)"""
    ws, bs = synthetic_params(dims, seed=seed)
    rw, rb, costs = [w * 0.1 for w in ws], bs, []
    for ep in range(2):
        for j in range(nb):
            xb = np.concatenate([X[j * Bs:(j + 1) * Bs] for X in Xs])
            yb = np.concatenate([Y[j * Bs:(j + 1) * Bs] for Y in Ys])
            rw, rb, c = oracle.train_batch(rw, rb, xb, yb, 3.0)
            if ep == 0:
                costs.append(c)
    return rw, rb, costs


# ---- tolerances and checks ---------------------------------------------------------------------------------------------------------------
# the resident kernel against the reference loop: one step from identical parameters, and six chained steps in a shuffled
# order -- (relative, absolute) of a parameter, relative of a cost
F32_ONE_STEP = (1e-5, 1e-6, 1e-5)
F32_SIX_STEPS = (1e-4, 1e-5, 1e-4)
F64_ONE_STEP = (1e-11, 1e-12, 1e-11)
F64_SIX_STEPS = (1e-10, 1e-11, 1e-10)


def close_to(got, want, tol, what):
    """every array of got within rel * |want| + ab of its counterpart, tol = (rel, ab, _)"""
    rel, ab, _ = tol
    for a, b in zip(got, want):
        err = np.abs(a - b) - (rel * np.abs(b) + ab)
        print(what, "largest |d| =", float(np.abs(a - b).max()), "over the bound by", float(err.max()))
        assert np.all(err <= 0.0), (what, float(np.abs(a - b).max()))


def same_bits(got, want, bits, what):
    """(parameters, per-step costs) pairs equal as `bits` patterns (+0 is not -0), the costs finite and positive on both sides.  A got
    without costs (None: a call that asked for none) is held on its parameters alone."""
    (got_p, got_c), (want_p, want_c) = got, want
    if got_c is not None:
        assert np.all(np.isfinite(want_c)) and want_c.min() > 0.0, f"{what}: the costs to equal are not those of a training step: {want_c}"
        assert np.all(np.isfinite(got_c)) and got_c.min() > 0.0, f"{what}: the costs are not those of a training step: {got_c}"
        assert np.array_equal(got_c.view(bits), want_c.view(bits)), f"{what}: per-step costs differ: {got_c - want_c}"
    assert np.array_equal(got_p.view(bits), want_p.view(bits)), f"{what}: parameters differ at {np.flatnonzero(got_p.view(bits) != want_p.view(bits))[:8]}"


# ---- feature nets and their contexts -----------------------------------------------------------------------------------------------------
def feature_net(input_shape, convpool, F, hidden=30, classes=10, **more):
    """convpool "default": the two convolve + pool pairs, (h / 4) (w / 4) 16 features; "one": one pair, (h / 2) (w / 2) 4"""
    return dict(input_shape=input_shape, convpool=convpool, F=F, hidden=hidden, classes=classes, **more)


FEATURE_NETS = {"784-30-10": feature_net((28, 28), "default", 784),     # the last feature worker holds ONE 16-feature slice
                "36-30-10": feature_net((6, 6), "one", 36)}             # three slices: worker 1 has a first slice and no second one
WHAT_STEPS = {"1step": 1, "3steps": 3, "5steps-2seg": 5, "begin": 3}    # the calls Pair.run knows by name


def index_of(perm, B, form):
    """a shuffled index, the same index entered one batch in, no index (stored order)"""
    return {"shuffled": perm, "offset": perm[B:], "stored": None}[form]


def make_rcn(spec, dtype, path=None, options=()):
    """a context of the feature net `spec`; path and options reach the library only where given (path 0 / None: its own selection)"""
    import mercer_research_amd as amd
    from mercer_research_amd.device import DeviceRCN
    L = amd.RCNLayer
    convpool = {"default": None, "one": [L.Convolve2D(amd.Padding.SAME), L.Pool2D(amd.Pooling.MAX)]}[spec["convpool"]]
    d = DeviceRCN(classes=spec["classes"], convpool_cfg=convpool, feedforward_cfg=[spec["hidden"]], input_shape=spec["input_shape"], dtype=dtype)
    assert d.F == spec["F"], (d.F, spec["F"])
    if path:
        d.set_dense_path(path)
    for k, v in dict(options).items():
        d.set_option(k, v)
    return d


def draw_rows(spec, dtype, rows, seed):
    """the data of the pair files, drawn from ONE generator in this order: X (rectified normals), Y (one-hot), perm"""
    rng = np.random.default_rng(seed)
    X = np.maximum(rng.standard_normal((rows, spec["F"])), 0.0).astype(NP_T[dtype])
    Y = np.eye(spec["classes"], dtype=NP_T[dtype])[rng.integers(0, spec["classes"], rows)]
    perm = rng.permutation(rows).astype(np.int32)
    return X, Y, perm


DP_GROUP_OF_ONE = "data-parallel at a group of one"


class Pair:
    """One feature net in one dtype: named contexts that differ in how they are formed, the starting parameters (synthetic_params of
    seed 42, weights x 0.1), and per context the data on the device.
    forms       ((name, form), ...): a form is a dict of options, or DP_GROUP_OF_ONE -- the data-parallel entry points at a group of one
                rank, bootstrapped over RCCL (the caller's fixture sets RCN_HIP_DP_P2P = 2; no bootstrap on the box: skip)
    data        the file's data policy, (spec, B) -> (rows, seed): draw_rows(spec, dtype, rows, seed) is what a call at batch B reads
    path        the dense path of every context (5: the resident kernel or an error)
    resident    every call asserts that the resident kernel answers at its batch size
    A spec with "unaligned" set has its feature matrix start one element into a longer buffer, 4 bytes off a 16-byte line."""

    def __init__(self, spec, dtype, forms, data, path=None, resident=False):
        import mercer_research_amd as amd
        self.spec, self.dtype, self.bits, self.policy, self.resident = spec, dtype, BITS[dtype], data, resident
        ws, bs = synthetic_params([spec["F"], spec["hidden"], spec["classes"]], seed=42)
        self.ws, self.bs = [w * 0.1 for w in ws], bs
        self.ctx, self.dp, self.host, self.data = {}, set(), {}, {}
        for name, form in forms:
            d = self.ctx[name] = make_rcn(spec, dtype, path, () if form == DP_GROUP_OF_ONE else form)
            if form == DP_GROUP_OF_ONE:
                try:
                    assert d.dp_init() == (0, 1), "a group of one is rank 0 of 1"
                except amd.RcnHipError as e:
                    pytest.skip(f"no RCCL bootstrap on this box: {e}")
                self.dp.add(name)
                assert d.dp_p2p_mode() == 2, d.dp_p2p_mode()
            else:
                for k, v in form.items():
                    assert d.get_option(k) == v, (name, k, d.get_option(k))

    def on_device(self, which, B):
        rows, seed = self.policy(self.spec, B)
        if (rows, seed) not in self.host:
            self.host[(rows, seed)] = draw_rows(self.spec, self.dtype, rows, seed)
        if (which, rows, seed) not in self.data:
            X, Y, perm = self.host[(rows, seed)]
            d = self.ctx[which]
            if self.spec.get("unaligned"):                       # the same rows one element into a longer buffer
                flat = d.to_device(np.concatenate([np.zeros(1, X.dtype), X.ravel(), np.zeros(3, X.dtype)]))
                Xd = flat[1:1 + X.size].view(rows, self.spec["F"])
                assert Xd.data_ptr() % 16 == 4 and Xd.is_contiguous(), Xd.data_ptr()
            else:
                Xd = d.to_device(X)
                assert Xd.data_ptr() % 16 == 0, Xd.data_ptr()
            self.data[(which, rows, seed)] = (Xd, d.to_device(Y), d.to_device(perm))
        return self.data[(which, rows, seed)] + (rows,)

    def run(self, which, B, form, what, cost=True):
        """-> (parameters, per-step costs | None) of one call from the starting parameters.  what: a number of steps through
        train_epoch, or a name of WHAT_STEPS -- then pack_segment_bytes is set, to two batches for "5steps-2seg" so that both halves of
        the image are used and re-packed in the call, and "begin" is epoch_begin + epoch_steps(0, 1) + epoch_steps(1, 2)."""
        d, dp = self.ctx[which], which in self.dp
        X, Y, perm, rows = self.on_device(which, B)
        nb = WHAT_STEPS[what] if isinstance(what, str) else what
        assert (nb + (form == "offset")) * B <= rows, f"{nb} steps of {B} ({form}) read past the {rows} rows this call owns"
        if self.resident:
            assert d.train_epoch_resident(B), f"{which}: the resident kernel does not answer at B = {B}"
            assert not dp or d.dp_resident(B), f"{which}: the data-parallel form is not resident at B = {B}"
        if isinstance(what, str):
            G = (self.spec["F"] + 15) // 16
            d.set_option("pack_segment_bytes", 2 * G * B * 16 * NP_T[self.dtype]().itemsize if what == "5steps-2seg" else 64 << 20)
        d.set_params(self.ws, self.bs)
        loss = d.empty(nb) if cost else None
        index = index_of(perm, B, form)
        if what == "begin":
            d.epoch_begin(X, Y, index, B, nb)
            d.epoch_steps(0, 1, 3.0, loss)
            d.epoch_steps(1, 2, 3.0, loss[1:] if cost else None)
        else:
            (d.dp_train_epoch if dp else d.train_epoch)(X, Y, index, B, nb, 3.0, loss)
        d.synchronize()
        assert d.fallbacks_taken() == 0, "a launch stepped down to another path"
        return d.params_flat().cpu().numpy().copy(), (loss.cpu().numpy().copy() if cost else None)

    def close(self):
        for name in self.dp:
            self.ctx[name].dp_finalize()
        for d in self.ctx.values():
            d.rcn.close()


def cached_pairs(make, dp_group_of_one=False):
    """-> a module-scope fixture: get(*key) is make(*key), made once per key and closed when the module is done.  dp_group_of_one: the
    module's contexts are created with the bootstrap over RCCL forced on (RCN_HIP_DP_P2P = 2)."""
    @pytest.fixture(scope="module")
    def fixture():
        made = {}
        with pytest.MonkeyPatch.context() as mp:
            if dp_group_of_one:
                mp.setenv("RCN_HIP_DP_P2P", "2")

            def get(*key, **kw):
                k = (key, repr(sorted(kw.items())))
                if k not in made:
                    made[k] = make(*key, **kw)
                return made[k]

            yield get
            for p in made.values():
                p.close()
    return fixture


# ---- one step in stored order, six chained steps shuffled, against the oracle -------------------------------------------------------------
def one_and_six_inputs(hidden, seed, dtype, N=2048):
    """-> X, Y, perm, ws, bs as f64, drawn in this order from ONE generator: X (rectified normals, rounded through dtype), Y (one-hot),
    perm; the parameters are synthetic_params of seed 21 with the weights x 0.1"""
    rng = np.random.default_rng(seed)
    X = np.maximum(rng.standard_normal((N, 784)), 0.0).astype(NP_T[dtype]).astype(np.float64)
    Y = one_hot(rng.integers(0, 10, N))
    ws, bs = synthetic_params([784] + hidden + [10], seed=21)
    perm = rng.permutation(N).astype(np.int32)
    return X, Y, perm, [w * 0.1 for w in ws], bs


def one_and_six_steps(d, ws, bs, Xd, Yd, pd, B, nb, runs=1, costless=False):
    """From (ws, bs): one step in stored order, then nb more in the order pd -> (parameters after one step, parameters after all, the
    1 + nb costs).  runs = 2: the same calls again give the same bits.  costless: the same calls without a cost buffer give the same
    parameters as bits.  No launch may step down."""
    got = []
    for _ in range(runs):
        d.set_params(ws, bs)
        loss = d.empty(nb + 1)
        d.train_epoch(Xd, Yd, None, B, 1, 3.0, loss)                   # one step, stored order
        p1 = sum(d.get_params(), [])
        d.train_epoch(Xd, Yd, pd, B, nb, 3.0, loss[1:])                 # nb more, shuffled
        d.synchronize()
        assert d.fallbacks_taken() == 0, "a launch stepped down to another path"
        flat = d.params_flat().cpu().numpy().copy() if runs > 1 or costless else None
        got.append((p1, sum(d.get_params(), []), loss.cpu().numpy().copy(), flat))
    bits = BITS[F64 if got[0][2].dtype == np.float64 else F32]
    for p1, _, costs, flat in got[1:]:
        assert np.array_equal(got[0][2].view(bits), costs.view(bits)), f"two runs of the same calls, costs differ: {got[0][2] - costs}"
        assert np.array_equal(got[0][3].view(bits), flat.view(bits)), "two runs of the same calls, parameters differ"
        for a, b in zip(got[0][0], p1):
            assert np.array_equal(np.asarray(a), np.asarray(b)), "two runs of the same calls, parameters after one step differ"
    if costless:
        d.set_params(ws, bs)
        d.train_epoch(Xd, Yd, None, B, 1, 3.0, None)
        d.train_epoch(Xd, Yd, pd, B, nb, 3.0, None)
        d.synchronize()
        assert d.fallbacks_taken() == 0, "a launch stepped down to another path"
        assert np.array_equal(got[0][3].view(bits), d.params_flat().cpu().numpy().view(bits)), "the parameters depend on whether a cost was asked for"
    return got[0][:3]


def check_one_and_six(oracle, got, ws, bs, X, Y, perm, B, nb, one_step, six_steps, costs_positive=False):
    """got: {name: one_and_six_steps(...)}.  Every entry against the oracle's train_batch on the same batches: the parameters and the
    cost after one step at the tolerance one_step, the nb chained steps at six_steps."""
    rw, rb, c0 = oracle.train_batch(ws, bs, X[:B], Y[:B], 3.0)
    for name, (p1, _, costs) in got.items():
        costs = costs.astype(np.float64)
        if costs_positive:
            assert np.all(np.isfinite(costs)) and costs.min() > 0.0, (name, costs)
        close_to(p1, rw + rb, one_step, f"{name}: one step")
        print(name, "cost of step 0:", costs[0], "oracle", c0)
        assert abs(costs[0] - c0) <= one_step[2] * c0, (name, costs[0], c0)
    rw, rb, cs = oracle_steps(oracle, rw, rb, X, Y, perm, B, nb, 3.0)
    for name, (_, p7, costs) in got.items():
        print(name, "costs of the chained steps:", costs[1:].tolist(), "oracle", cs.tolist())
        np.testing.assert_allclose(costs[1:].astype(np.float64), cs, rtol=six_steps[2], err_msg=str(name))
        close_to(p7, rw + rb, six_steps, f"{name}: {nb} chained steps")


# ---- rank processes ----------------------------------------------------------------------------------------------------------------------
def spawn_ranks(tmp_path, world, dtype, case_name, env_extra, *, dims, Bs, nb, seed=17):
    """`world` processes of tests/_p2p_worker.py on this box's GPU, rank r on the shard (X_r, Y_r) drawn here -> (Xs, Ys, the tails of
    the ranks' logs).  case_name None: the worker is started without one (its "default")."""
    rng = np.random.default_rng(31)
    dims = list(dims)
    Xs = [np.maximum(rng.standard_normal((Bs * nb, dims[0])), 0.0) for _ in range(world)]
    Ys = [one_hot(rng.integers(0, dims[-1], Bs * nb), dims[-1]) for _ in range(world)]
    np.savez(tmp_path / "case.npz", dims=dims, Bs=Bs, nb=nb, seed=seed, **{f"X{r}": Xs[r] for r in range(world)}, **{f"Y{r}": Ys[r] for r in range(world)})
    with socket.socket() as so:
        so.bind(("127.0.0.1", 0))
        port = so.getsockname()[1]
    worker = os.path.join(ROOT, "tests", "_p2p_worker.py")
    env = dict(os.environ, HSA_ENABLE_IPC_MODE_LEGACY="0", **env_extra)
    case = [] if case_name is None else [case_name]
    procs = [subprocess.Popen([sys.executable, worker, str(r), str(world), str(port), str(dtype), str(tmp_path)] + case, env=env,
                              stdout=subprocess.PIPE, stderr=subprocess.STDOUT) for r in range(world)]
    logs = []
    for pr in procs:
        try:
            out, _ = pr.communicate(timeout=240)
        except subprocess.TimeoutExpired:
            pr.kill()
            out, _ = pr.communicate()
        logs.append(out.decode(errors="replace")[-3000:])
    assert all(pr.returncode == 0 for pr in procs), "\n----\n".join(logs)
    return Xs, Ys, logs
