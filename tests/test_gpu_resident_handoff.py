"""The resident one-XCD kernel computes the same BITS as the commit tests/golden/resident_handoff_digests.json was recorded on
(tests/golden/make_resident_handoff_digests.py, run on the GPU): parameters and per-step costs after 3 and after 130 steps, for every
instantiation of k_xcd_epoch -- f32 at B in {10, 32, 64, 100, 128, 200, 256}, f64 at B in {10, 32, 128, 256} on 784-30-10, f32 at
B in {32, 256} on 784-10-10-10, and the data-parallel form at a group of one at B = 256.

How a step's hand-offs are scheduled (which wave waits for which flag, when delta_1 is staged) must change neither an operand nor an
order of summation, so the comparison is for equality of digests, not within a tolerance.  Nothing here sets a fault option.
"""
import importlib.util
import json
import os

import pytest

pytestmark = pytest.mark.gpu
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")

_spec = importlib.util.spec_from_file_location("make_resident_handoff_digests", os.path.join(GOLDEN, "make_resident_handoff_digests.py"))
maker = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(maker)

with open(os.path.join(GOLDEN, "resident_handoff_digests.json")) as _f:
    RECORDED = json.load(_f)
CASES = maker.cases()


def test_every_case_of_the_recipe_is_recorded():
    assert sorted(c["id"] for c in CASES) == sorted(RECORDED)


@pytest.mark.parametrize("case", CASES, ids=[c["id"] for c in CASES])
def test_resident_kernel_computes_the_recorded_bits(case):
    want = RECORDED[case["id"]]
    got = maker.run_case(case)
    print(case["id"], "params", got["params_sha256"], "loss", got["loss_sha256"])
    assert got["loss_head"] == want["loss_head"], "the first steps' costs differ"
    assert got["params_head"] == want["params_head"], "the first parameters differ"
    assert got["loss_sha256"] == want["loss_sha256"], "the per-step costs differ somewhere past the first 16"
    assert got["params_sha256"] == want["params_sha256"], "the parameters differ somewhere past the first 16"
