"""CPU tests of Track X's evaluation metrics (include/rcn_hipx.h, rcn_hipx_evaluate_metrics_dev): the rank rule on the host
(rcn_hipx_label_rank, the function k_eval_metrics runs) against the NumPy restatement tests/_eval_ref.py, the restatement against torch.topk
and a plain double loop, the host side of EvalReport, and the plain evaluation plans, which this feature leaves byte for byte what they
were (tests/golden/plan_eval_texts.json, recorded before k_eval_metrics existed).  No GPU needed, none touched; the plan of a metrics
chunk needs a net handle and is held by tests/test_gpu_convnet_eval_metrics.py."""
import ctypes as C
import json
import os

import _eval_ref
import numpy as np
import pytest
from _convnet_util import CIFAR, FUSED_HEAD, MNIST, ODD_WIDTH, PLAIN_HEAD, POOL_PAIRS, convnet_loaded  # noqa: F401  (convnet_loaded: the fixture `convnet`)

CLASSES = (1, 7, 10, 32, 33, 40)
PLAN_SPECS = {"fused_head": FUSED_HEAD, "plain_head": PLAIN_HEAD, "pool_pairs": POOL_PAIRS, "odd_width": ODD_WIDTH, "cifar": CIFAR, "mnist": MNIST}
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "plan_eval_texts.json")


def _rows(rng, kind, n, classes):
    if kind == "gaussian":
        return rng.standard_normal((n, classes)).astype(np.float32)
    if kind == "ties":                                                # three integer values: many equal logits in every row
        return rng.integers(-1, 2, (n, classes)).astype(np.float32)
    z = rng.standard_normal((n, classes)).astype(np.float32)         # "inf": about a third of the entries +inf or -inf
    pick = rng.integers(0, 6, (n, classes))
    z[pick == 0], z[pick == 1] = np.inf, -np.inf
    return z


@pytest.mark.parametrize("kind", ["gaussian", "ties", "inf"])
@pytest.mark.parametrize("classes", CLASSES)
def test_label_rank_is_the_restatement(convnet, classes, kind):
    rng = np.random.default_rng(classes * 7 + len(kind))
    n = 40
    z = _rows(rng, kind, n, classes)
    y = rng.integers(0, classes, n).astype(np.int32)
    want = _eval_ref.rank(z, y)
    got = np.array([convnet.label_rank(z[i], int(y[i])) for i in range(n)], dtype=np.int32)
    assert np.array_equal(got, want), (got, want)
    assert want.min() >= 0 and want.max() <= classes - 1
    if kind == "ties" and classes >= 7:
        assert len(set(want.tolist())) >= 3                          # the ranks are spread, not all 0
    # every label of one row: the ranks are a permutation of 0 .. classes - 1 (a stable descending sort places every class once)
    every = np.array([convnet.label_rank(z[0], c) for c in range(classes)])
    assert sorted(every.tolist()) == list(range(classes)), every
    assert np.array_equal(np.argsort(-z[0].astype(np.float64), kind="stable"), np.argsort(every))
    # a label outside [0, classes): -1 from both, and nothing is indexed
    for bad in (-1, classes, classes + 1000, -2 ** 31, 2 ** 31 - 1):
        assert convnet.label_rank(z[0], bad) == -1
        assert _eval_ref.rank(z[:1], np.array([bad]))[0] == -1


def test_label_rank_refuses_null_and_empty_rows(convnet):
    lib = convnet.load()
    row = (C.c_float * 4)(1.0, 2.0, 3.0, 4.0)
    out = C.c_int(77)
    assert lib.rcn_hipx_label_rank(None, 4, 1, C.byref(out)) == -1
    assert lib.rcn_hipx_label_rank(row, 4, 1, None) == -1
    assert lib.rcn_hipx_label_rank(row, 0, 0, C.byref(out)) == -1 and lib.rcn_hipx_label_rank(row, -3, 0, C.byref(out)) == -1
    assert out.value == 77                                            # a refusal writes nothing
    assert lib.rcn_hipx_label_rank(row, 4, 1, C.byref(out)) == 0 and out.value == 2
    with pytest.raises(ValueError):
        convnet.label_rank(np.zeros(0, dtype=np.float32), 0)


@pytest.mark.parametrize("classes", [c for c in CLASSES if c > 1])
def test_rank_below_k_is_torch_topk_membership_on_rows_without_ties(classes):
    import torch
    rng = np.random.default_rng(classes)
    n = 64
    z = rng.standard_normal((n, classes))                             # float64: no two entries of a row are equal
    assert all(len(set(r.tolist())) == classes for r in z)
    y = rng.integers(0, classes, n)
    r = _eval_ref.rank(z, y)
    for k in sorted({1, 2, min(5, classes), classes}):
        idx = torch.topk(torch.from_numpy(z), k, dim=1).indices.numpy()
        member = (idx == y[:, None]).any(axis=1)
        assert np.array_equal(r < k, member), k
        assert _eval_ref.topk_counts(r, [k])[0] == int(member.sum())
    assert np.array_equal(r == 0, _eval_ref.pred(z) == y)


def test_confusion_is_the_plain_double_loop():
    rng = np.random.default_rng(5)
    classes, n = 7, 200
    y = rng.integers(-1, classes + 1, n)                              # some labels out of range
    p = rng.integers(0, classes, n)
    want = np.zeros((classes, classes), dtype=np.int64)
    for a in range(classes):
        for b in range(classes):
            want[a, b] = sum(1 for i in range(n) if y[i] == a and p[i] == b)
    got = _eval_ref.confusion(y, p, classes)
    assert np.array_equal(got, want)
    assert got.sum() == int(((y >= 0) & (y < classes)).sum()) < n


def test_loss_sum_from_rows_follows_the_documented_order():
    """chunks of max_batch rows, blocks of 8 in float32, 256 strided float64 sums: against the order spelled out by hand on a case where
    a float32 block sum differs from the float64 one"""
    rows = np.array([1.0, 2.0 ** -24, 2.0 ** -24, 2.0 ** -24, 0, 0, 0, 0, 2.0 ** -24, 5.0, 7.0], dtype=np.float32)
    b0 = np.float32(1.0)                                              # 1 + 2^-24 rounds back to 1 in float32, three times
    b1 = np.float32(np.float32(np.float32(2.0 ** -24) + np.float32(5.0)) + np.float32(7.0))
    assert _eval_ref.loss_sum_from_rows(rows, 16) == np.float64(b0) + np.float64(b1)
    assert _eval_ref.loss_sum_from_rows(rows, 16) != rows.astype(np.float64).sum()
    # max_batch 9: the second chunk begins at row 9, so row 8 is a block of its own
    c0 = np.float64(b0) + np.float64(np.float32(2.0 ** -24))
    c1 = np.float64(np.float32(np.float32(5.0) + np.float32(7.0)))
    assert _eval_ref.loss_sum_from_rows(rows, 9) == c0 + c1
    # more than 256 blocks in a chunk: "thread" 0 takes blocks 0 and 256 before the 256 sums are added in order
    many = np.zeros(8 * 257, dtype=np.float32)
    many[0], many[8], many[8 * 256] = 1.0, 2.0 ** -53, 2.0 ** -53
    assert _eval_ref.loss_sum_from_rows(many, 8 * 257) == (np.float64(1.0) + 2.0 ** -53) + 2.0 ** -53 == 1.0
    many[0], many[8 * 256] = 2.0 ** -53, 1.0
    assert _eval_ref.loss_sum_from_rows(many, 8 * 257) == (np.float64(2.0 ** -53) + 1.0) + 2.0 ** -53 == 1.0
    many[0], many[8], many[16], many[8 * 256] = 1.0, 2.0 ** -53, 2.0 ** -53, 0.0
    assert _eval_ref.loss_sum_from_rows(many, 8 * 257) == 1.0         # ((1 + 2^-53) + 2^-53): each addition rounds back to 1


def test_eval_report_helpers(convnet):
    m = np.array([[3, 1, 0], [0, 0, 0], [2, 0, 4]], dtype=np.int64)   # class 1 has no rows; it is predicted once
    rep = convnet.EvalReport(n=10, loss=0.5, correct=7, topk={1: 7}, confusion=m)
    assert rep.accuracy() == 0.7
    rec, pre = rep.recall(), rep.precision()
    assert rec[0] == 0.75 and np.isnan(rec[1]) and rec[2] == 4 / 6
    assert pre[0] == 0.6 and pre[1] == 0.0 and pre[2] == 1.0
    never = convnet.EvalReport(n=1, loss=0.0, correct=1, topk={}, confusion=np.array([[1, 0], [0, 0]], dtype=np.int64))
    assert np.isnan(never.precision()[1]) and np.isnan(never.recall()[1])
    empty = convnet.EvalReport(n=0, loss=0.0, correct=0, topk={}, confusion=np.zeros((2, 2), dtype=np.int64))
    assert np.isnan(empty.accuracy())
    with pytest.raises(ValueError):
        convnet.EvalReport(n=1, loss=0.0, correct=0, topk={}).accuracy()


def test_plan_eval_metrics_net_refuses_what_it_cannot_walk(convnet):
    lib = convnet.load()
    buf = C.create_string_buffer(256)
    assert lib.rcn_hipx_plan_eval_metrics_net(None, 1, 2, 1, 0, 0, buf, len(buf)) == -1


def test_plain_evaluation_plans_are_what_they_were(convnet):
    """rcn_hipx_plan_eval over the shared specs in every precision: the texts (or the refusals) recorded before this feature"""
    with open(GOLDEN) as f:
        golden = json.load(f)
    seen = 0
    for name, (shp, layers, B) in PLAN_SPECS.items():
        for precision in ("fp32", "bf16", "bf16_stored"):
            try:
                text = convnet.plan_eval(shp, layers, B, precision, "auto")
            except convnet.ConvNetError as e:
                text = "refused: " + str(e)
            assert text == golden[f"{name}-{precision}"], (name, precision)
            assert "k_eval_metrics" not in text
            seen += "k_eval_ce" in text
    assert len(golden) == 3 * len(PLAN_SPECS) and seen >= 2 * len(PLAN_SPECS)
