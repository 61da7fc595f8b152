"""CPU proofs behind tests/test_gpu_convnet_exact.py (tests/_exact_nets.py), from the oracle alone -- no GPU, and the library only for
the plan that says which nets it accepts under bf16 storage (every net runs in bf16 and, where accepted, under bf16 storage):
  1  every (net, precision) the GPU file runs is certified: operands on one power-of-two quantum, every GEMM's sum of absolute terms below
     2**20 quanta, and in the bf16 modes the oracle with rounded operands / stored maps gives the f64 logits -- so "bit for bit" is what
     the device owes.  The gradient cases keep a logit gap of at most 16; the saturated ones lie in [120, 600].
  2  the data does what Gaussian data never does: at least 30 pooling windows tied at a positive maximum (nets with a pool) and at least 30
     pre-activations exactly 0.
  3  the GPU comparison would fail a wrong rule: an oracle that routes a tied window to its LAST maximum, and one whose gate is >= 0, each
     move some gradient tensor by more than ten times the mode's tolerance of that tensor's scale.  The restated walk those mutants live
     in is the oracle bit for bit with the rules as they are.
  4  the oracle's conventions (padding 1, tap order k = (kh*3+kw)*Cin + ci, NHWC flatten, first maximum, gate > 0) are torch's: float64
     conv2d / max_pool2d / relu / cross_entropy with autograd agree with it within 1e-12 on an exact net, where ties and zeros are real;
     with label smoothing 0.1 against tests/_mix_ref.soft_loss_and_grads.  Finite differences (tests/test_convnet_oracle.py) cannot see these.

Measured (printed by the tests; seed 0 everywhere):
  largest sum of absolute terms over all cases: 337 quanta (the bf16-storage forms net), against the bound 2**20
  logit_shift 1 to 5 for the gradient cases (gaps 8.5 to 16), 0, -1 and -3 for the saturated ones (gaps 160, 160, 176)
  tied windows / zero pre-activations in the smallest case: 52 / 327 (bf16-dense-nk's net); the 4 x 8 remap nets have no pool, so no
  window (1995 zeros at least)
  rows of the evaluation sets whose two largest logits are equal: 0, 0 and 3 (POOL_PAIRS: the first-maximum rule of predict is exercised)
  mutants, move of the most-moved tensor as a fraction of that tensor's scale, smallest .. largest over the backward cases:
    last maximum  fp32 0.267 .. 0.886 (18 cases)   bf16 0.384 .. 0.756 (9)   bf16 storage 0.267 .. 0.411 (3)
    gate >= 0     fp32 0.151 .. 1.03  (19)         bf16 0.247 .. 1.03  (10)  bf16 storage 0.151 .. 0.569 (3)
  against 10 x tolerance = 2e-3 (fp32) and 5e-2 (bf16 modes).
  5  the exact BACKWARD cases (_exact_nets.BACKWARD_CASES: tied classes at the maximum, the others 120 or more below, power-of-two batches):
     every (net, precision) is certified forward and backward -- every backward GEMM on one quantum with its sum of absolute terms below
     2**20 quanta, the walk the same array in the mode as in f64, every reference array float32 values, the f64 softmax within 2**-149 of
     the limit 1/t | 0 the walk starts from; dZ is alive in every convolution layer (COVERAGE); and every mutant -- last maximum, gate at
     zero, per convolution layer an input gradient without dZ's last row, last column, last image or without ONE tap at one pixel and
     channel, and a weight gradient without dZ's last live pixel of the last image or without the last image -- changes at least one tensor of the gradient, which an exact comparison
     then tells.  The plans name the backward kernel forms each case is there for.
  Measured: largest backward sum 18606 quanta (the 3-class net at a batch of 128), elsewhere 52 to 9339."""
import numpy as np
import pytest
from _convnet_util import FUSED_HEAD, HALO_NETS, PLAIN_HEAD, POOL_PAIRS, convnet_loaded  # noqa: F401  (convnet_loaded: the fixture `convnet`)
from _exact_nets import (BACKWARD_CASES, COVERAGE, EVAL_ROWS, MODES, STORED_TILING, backward_case, backward_certificate, certificate, coverage, degeneracy,
                         eval_set, exact_case, gpu_cases, logit_gap, mutants, one_hot, plain_nets, walk, worst_move)
from _forms_cases import DENSE_NK, env_name, names
from _mix_ref import soft_loss_and_grads, soft_targets

from oracle import convnet_oracle as co


def _unique(cases):
    seen, out = set(), []
    for c in cases:
        if (c.spec, c.precision) not in seen:
            seen.add((c.spec, c.precision))
            out.append(pytest.param(c.spec, c.precision, id=c.id))
    return out


ALL = _unique(gpu_cases())
BACKWARD = _unique([c for c in gpu_cases() if c.backward])
SATURATED = [FUSED_HEAD, PLAIN_HEAD, DENSE_NK]
EVALUATED = [FUSED_HEAD, PLAIN_HEAD, POOL_PAIRS]


def _has_pool(layers):
    return any(l[0] == "pool" for l in layers)


def test_every_forms_case_and_every_plain_net_is_a_case():
    ids = [c.id for c in gpu_cases()]
    assert len(ids) == len(set(ids)), ids
    assert len(ALL) >= 30 and len(BACKWARD) >= 25, (len(ALL), len(BACKWARD))


def test_bf16_storage_runs_wherever_the_library_accepts_the_net(convnet):
    """STORED_TILING against the plan: every net in it is accepted at its tiling, every other net is refused at "auto" and at "lds";
    every net is accepted in bf16 at its own tiling.  So the GPU file leaves out no (net, mode) that could run."""
    def accepted(spec, precision, tiling):
        try:
            convnet.plan(*spec, precision=precision, tiling=tiling or "auto")
            return True
        except convnet.ConvNetError as e:
            assert "bf16 storage" in str(e), e
            return False
    cases = {(c.spec, c.precision) for c in gpu_cases()}
    for name, spec, tiling in plain_nets():
        assert accepted(spec, "bf16", tiling) and (spec, "bf16") in cases, name
        if spec in STORED_TILING:
            assert accepted(spec, "bf16_stored", STORED_TILING[spec]) and (spec, "bf16_stored") in cases, name
            assert STORED_TILING[spec] is None or tiling == "lds" or not accepted(spec, "bf16_stored", None), name
        else:
            assert not accepted(spec, "bf16_stored", None) and not accepted(spec, "bf16_stored", "lds"), name
    assert not set(STORED_TILING) - {s for _, s, _ in plain_nets()}


@pytest.mark.parametrize("spec,precision", ALL)
def test_case_is_certified_and_its_data_ties_and_hits_zero(spec, precision):
    _, layers, _ = spec
    case = exact_case(spec)
    worst = certificate(case.x, list(case.ws), list(case.bs), layers, precision)
    ties, zeros = degeneracy(case.x, list(case.ws), list(case.bs), layers)
    print(f"{precision}: largest sum {worst:.0f} quanta; logit_shift {case.shift}, gap {case.gap}; tied windows {ties}; zero pre-activations {zeros}")
    assert case.gap <= 16, case.gap
    if _has_pool(layers):
        assert ties >= 30, ties
    assert sum(zeros) >= 30, zeros


@pytest.mark.parametrize("spec,precision", BACKWARD)
def test_a_last_maximum_or_a_gate_at_zero_would_fail_the_gpu_comparison(spec, precision):
    _, layers, _ = spec
    kw, rtol = MODES[precision]
    case = exact_case(spec)
    x64, ws, bs = case.x.astype(np.float64), list(case.ws), list(case.bs)
    T = one_hot(case.y, layers[-1][1])
    loss, logits, gws, gbs = walk(x64, T, ws, bs, layers, **kw)
    # the walk with the rules as they are IS the oracle
    o_loss, o_logits, o_gws, o_gbs = co.loss_and_grads(x64, case.y, ws, bs, layers, **kw)
    assert loss == o_loss and np.array_equal(logits, o_logits)
    assert all(np.array_equal(a, b) for a, b in zip(gws + gbs, o_gws + o_gbs))
    mutants = [dict(gate=">=")] + ([dict(tie="last")] if _has_pool(layers) else [])
    for m in mutants:
        _, m_logits, m_gws, m_gbs = walk(x64, T, ws, bs, layers, **kw, **m)
        assert np.array_equal(m_logits, logits)                    # neither rule changes the forward pass
        moved = worst_move(m_gws, m_gbs, gws, gbs)
        print(f"{precision} {m}: most-moved tensor by {moved:.3g} of its scale; 10 x tolerance = {10 * rtol:g}")
        assert moved > 10 * rtol, (m, moved)


@pytest.mark.parametrize("spec", SATURATED, ids=["fused_head", "plain_head", "dense_nk"])
def test_saturated_cases_are_certified_with_a_gap_where_expf_underflows(spec):
    _, layers, _ = spec
    case = exact_case(spec, "saturated")
    worst = certificate(case.x, list(case.ws), list(case.bs), layers, "fp32")
    print(f"largest sum {worst:.0f} quanta; logit_shift {case.shift}, gap {case.gap}")
    assert 120 <= case.gap <= 600, case.gap
    z = case.logits - case.logits.max(axis=1, keepdims=True)
    assert (np.exp(z.astype(np.float32)) == 0).any()               # float32 exp does underflow to 0 on these logits
    assert ((0 <= case.y) & (case.y < layers[-1][1])).all()


@pytest.mark.parametrize("spec", EVALUATED, ids=["fused_head", "plain_head", "pool_pairs"])
def test_evaluation_sets_are_certified(spec):
    _, layers, B = spec
    assert EVAL_ROWS[spec] % B
    case = exact_case(spec)
    X, _ = eval_set(spec)
    x = X.astype(np.float64) - 2.0
    worst = certificate(x, list(case.ws), list(case.bs), layers, "fp32")
    logits = co.forward(x, list(case.ws), list(case.bs), layers)
    tied = int((np.sort(logits, axis=1)[:, -1] == np.sort(logits, axis=1)[:, -2]).sum())
    print(f"largest sum {worst:.0f} quanta; gap {logit_gap(logits)}; rows whose two largest logits are equal: {tied}")


# ---- 4. the oracle's conventions are torch's -------------------------------------------------------------------------------------------------

def _torch_net(x, ws, bs, layers, y, smoothing):
    import torch
    import torch.nn.functional as F
    t = torch.from_numpy(np.ascontiguousarray(np.asarray(x, dtype=np.float64).transpose(0, 3, 1, 2)))
    params, pi = [], 0
    for l in layers:
        if l[0] == "conv":
            cin = t.shape[1]
            w = torch.from_numpy(np.ascontiguousarray(ws[pi].reshape(3, 3, cin, l[1]).transpose(3, 2, 0, 1))).requires_grad_()
            b = torch.from_numpy(bs[pi].copy()).requires_grad_()
            t = F.relu(F.conv2d(t, w, b, padding=1))
        elif l[0] == "pool":
            t = F.max_pool2d(t, 2)
            continue
        else:
            if t.dim() == 4:
                t = t.permute(0, 2, 3, 1).reshape(t.shape[0], -1)      # NHWC flatten
            w = torch.from_numpy(ws[pi].copy()).requires_grad_()
            b = torch.from_numpy(bs[pi].copy()).requires_grad_()
            t = t @ w + b
            if l[0] == "dense_relu":
                t = F.relu(t)
        params.append((l[0], w, b)); pi += 1
    loss = F.cross_entropy(t, torch.from_numpy(np.asarray(y, dtype=np.int64)), label_smoothing=smoothing)
    loss.backward()
    gws = [w.grad.numpy().transpose(2, 3, 1, 0).reshape(-1, w.shape[0]) if kind == "conv" else w.grad.numpy() for kind, w, _ in params]
    return float(loss.detach()), t.detach().numpy(), gws, [b.grad.numpy() for _, _, b in params]


@pytest.mark.parametrize("smoothing", [0.0, 0.1])
def test_oracle_is_torch_on_an_exact_net(smoothing):
    """conv-conv-pool, a convolution without a pool, a ReLU dense layer and the logits layer: HALO_NETS[2]"""
    spec = HALO_NETS[2]
    _, layers, _ = spec
    case = exact_case(spec)
    x64, ws, bs = case.x.astype(np.float64), list(case.ws), list(case.bs)
    ties, zeros = degeneracy(x64, ws, bs, layers)
    assert ties >= 30 and sum(zeros) >= 30, (ties, zeros)
    if smoothing == 0.0:
        loss, logits, gws, gbs = co.loss_and_grads(x64, case.y, ws, bs, layers)
    else:
        loss, logits, gws, gbs = soft_loss_and_grads(x64, soft_targets(case.y, case.y, 1.0, smoothing, layers[-1][1]), ws, bs, layers)
    t_loss, t_logits, t_gws, t_gbs = _torch_net(x64, ws, bs, layers, case.y, smoothing)
    assert np.array_equal(t_logits, logits)                          # exact arithmetic: not one bit apart
    assert abs(t_loss - loss) <= 1e-12 * abs(loss), (t_loss, loss)
    for k, (a, b) in enumerate(zip(t_gws + t_gbs, gws + gbs)):
        d, scale = float(np.abs(a - b).max()), float(np.abs(b).max())
        print("tensor", k, "max |d| =", d, "scale =", scale)
        assert a.shape == b.shape and d <= 1e-12 * scale, (k, d, scale)


# ---- 5. the exact backward cases -------------------------------------------------------------------------------------------------------------

def _backward_nets():
    """(spec, extra) -> the precisions its cases run in"""
    nets = {}
    for c in BACKWARD_CASES:
        modes = nets.setdefault((c.spec, c.extra), [])
        if c.precision not in modes:
            modes.append(c.precision)
    return [pytest.param(spec, extra, tuple(modes), id=next(c.id for c in BACKWARD_CASES if (c.spec, c.extra) == (spec, extra))) for (spec, extra), modes in nets.items()]


def test_backward_cases_cover_what_the_suite_promises():
    ids = [c.id for c in BACKWARD_CASES]
    assert len(ids) == len(set(ids)), ids
    assert all(c.spec[2] & (c.spec[2] - 1) == 0 for c in BACKWARD_CASES)
    for extra, least in (("sgd", 3), ("ema", 2), ("accum", 2), ("soft", 2)):
        assert sum(c.extra == extra for c in BACKWARD_CASES) >= least, extra
    assert {c.precision for c in BACKWARD_CASES if c.extra == "sgd"} == set(MODES)


@pytest.mark.parametrize("spec,extra,modes", _backward_nets())
def test_backward_case_is_certified_alive_and_tells_every_mutant(spec, extra, modes):
    _, layers, _ = spec
    c = backward_case(spec, extra)
    assert ((c.t <= c.y) & (c.y < layers[-1][1])).all()             # labels among the classes pushed down
    for mode in modes:
        worst = backward_certificate(c, mode)
        print(f"{mode}: largest backward sum {worst:.0f} quanta; push {c.push}, t {c.t}, loss {c.loss:.6g}")
    for pi, shares in coverage(c):
        print(f"parameter layer {pi}: dZ != 0 at", {k: round(v, 3) for k, v in shares.items()}, "least:", COVERAGE)
    if extra != "soft":
        # the flagged walk with its OWN softmax is still the oracle, bit for bit, on these values too
        x64, ws, bs = c.x.astype(np.float64), list(c.ws), list(c.bs)
        loss, logits, gws, gbs = walk(x64, c.T, ws, bs, layers)
        with np.errstate(divide="ignore"):                          # (f64's exp underflows too where the gap is above 745: both losses are inf)
            o_loss, o_logits, o_gws, o_gbs = co.loss_and_grads(x64, c.y, ws, bs, layers)
        assert loss == o_loss and np.array_equal(logits, o_logits) and all(np.array_equal(a, b) for a, b in zip(gws + gbs, o_gws + o_gbs))
    for mode in modes:
        for flags, changed in mutants(c, mode):
            assert changed, (mode, flags, "the mutant changes no tensor of the gradient")


@pytest.mark.parametrize("case", BACKWARD_CASES, ids=[c.id for c in BACKWARD_CASES])
def test_backward_case_plan_names_its_kernel_forms(convnet, monkeypatch, case):
    for name, value in case.options.items():
        monkeypatch.setenv(env_name(name), str(value))
    L = convnet.plan(*case.spec, precision=case.precision, tiling=case.tiling or "auto").splitlines()
    assert case.lines, case.id
    for text in case.lines:
        assert any(names(l, text) for l in L), (text, L)
