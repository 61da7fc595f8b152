"""CPU tests of Track X's evaluation pass through rcn_hipx_plan_eval: the dispatch code of ONE evaluation chunk run with every launch
replaced by a note (no GPU needed, none touched).  Evaluation runs the training step's own forward launches and then k_eval_ce; the
numerics are the GPU tests' business (tests/test_gpu_convnet_epoch.py)."""
import ctypes as C
import re

import pytest
from _convnet_util import convnet_built, plan_lines  # noqa: F401  (convnet_built: the fixture `convnet`)

from bench_convnet import CONFIGS

PRECISIONS = ("fp32", "bf16", "bf16_stored")


def _forward_part(lines):
    """A training plan up to (not including) its loss launch: the fused head or k_softmax_ce."""
    for i, l in enumerate(lines):
        if "k_head_f32" in l or "k_softmax_ce" in l:
            return lines[:i]
    raise AssertionError("a training plan without a loss launch")


@pytest.mark.parametrize("precision", PRECISIONS)
@pytest.mark.parametrize("config", list(CONFIGS))
def test_evaluation_runs_the_training_plans_forward_launches_and_one_eval_kernel(convnet, config, precision):
    shp, layers, B = CONFIGS[config]
    try:
        train = plan_lines(convnet.plan(shp, layers, B, precision, "auto"))
    except convnet.ConvNetError as e:
        if "rcn_hipx_plan: -3" in str(e):
            pytest.skip("rcn_hipx_plan itself refuses this pair")
        raise
    ev = plan_lines(convnet.plan_eval(shp, layers, B, precision, "auto"))
    keep = lambda ls: [l for l in ls if l.startswith("conv3x3") or l.startswith("pool")]
    assert keep(ev) == keep(_forward_part(train)) and len(keep(ev)) >= 2
    if precision != "fp32":
        assert ev[0].startswith("bf16 operand copies") and ev[0] == train[0]
    else:
        assert not any("bf16 operand copies" in l for l in ev)
    assert sum("k_eval_ce" in l for l in ev) == 1 and "k_eval_ce" in ev[-1]
    m = re.search(r"k_eval_ce, (\d+) workgroups", ev[-1])
    assert m and int(m.group(1)) == (B + 7) // 8                       # eight samples per workgroup, k_softmax_ce's grouping
    assert not any(l.startswith(("wgrad", "dgrad", "update")) for l in ev)
    assert not any(re.search(r"k_head_f32|k_softmax_ce|k_reduce_all", l) for l in ev)
    # the logits layer is one more forward launch (for a fused-head net the training plan has it inside k_head_f32)
    assert sum(l.startswith("dense") for l in ev) == sum(1 for l in layers if l[0] in ("dense", "dense_relu"))


def test_eval_workgroups_follow_the_batch(convnet):
    shp, layers, _ = CONFIGS["mnist"]
    for B in (1, 8, 9, 4096):
        last = plan_lines(convnet.plan_eval(shp, layers, B, "fp32", "auto"))[-1]
        assert f"k_eval_ce, {(B + 7) // 8} workgroups" in last, last


def test_plan_eval_reports_shape_errors_like_plan(convnet):
    lib = convnet.load()
    arr = (convnet.XLayer * 2)()
    arr[0].kind, arr[0].out = convnet.KIND["conv"], 48                                             # not a multiple of 32
    arr[1].kind, arr[1].out = convnet.KIND["dense"], 10
    buf, ref = C.create_string_buffer(4096), C.create_string_buffer(4096)
    assert lib.rcn_hipx_plan_eval(8, 8, 3, arr, 2, 4, 0, 1, buf, len(buf)) == -3
    assert lib.rcn_hipx_plan(8, 8, 3, arr, 2, 4, 0, 1, ref, len(ref)) == -3
    assert b"multiple of 32" in buf.value and buf.value == ref.value
    buf.value = ref.value = b"untouched"
    assert lib.rcn_hipx_plan_eval(8, 8, 3, arr, 2, 4, 7, 1, buf, len(buf)) == -1
    assert lib.rcn_hipx_plan(8, 8, 3, arr, 2, 4, 7, 1, ref, len(ref)) == -1
    assert buf.value == ref.value == b"untouched"


def test_plan_eval_refuses_bf16_storage_where_set_precision_would(convnet):
    """A net whose maps are too small for the bf16-tensor weight gradient cannot enter RCN_HIPX_BF16_STORED; its evaluation plan says so
    with rcn_hipx_plan's text."""
    net = ((8, 8, 3), (("conv", 32), ("pool",), ("conv", 64), ("pool",), ("dense", 10)), 16)
    with pytest.raises(convnet.ConvNetError, match="bf16 storage") as e_eval:
        convnet.plan_eval(*net, precision="bf16_stored")
    with pytest.raises(convnet.ConvNetError, match="bf16 storage") as e_plan:
        convnet.plan(*net, precision="bf16_stored")
    assert str(e_eval.value).split(": ", 2)[2] == str(e_plan.value).split(": ", 2)[2]
    assert "k_eval_ce" in convnet.plan_eval(*net, precision="bf16")


def test_epoch_entry_points_refuse_null_nets_without_a_gpu(convnet):
    lib = convnet.load()
    c = C.c_int64(5)
    assert lib.rcn_hipx_graphs_instantiated(None, C.byref(c)) == -1 and c.value == 5
    assert lib.rcn_hipx_train_epoch_dev(None, None, 0, 1.0, 0.0, None, 1, None, 1, 0, 1, 0.1, None) == -1
    assert lib.rcn_hipx_evaluate_dev(None, None, 0, 1.0, 0.0, None, 1, None, None, None) == -1
    buf = C.create_string_buffer(64)
    assert lib.rcn_hipx_plan_eval_net(None, 1, buf, len(buf)) == -1
