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
import pytest
from _rcn_util import (DP_GROUP_OF_ONE, F32, F32_ONE_STEP, F32_SIX_STEPS, FEATURE_NETS, Pair, cached_pairs, check_one_and_six, one_and_six_inputs,
                       one_and_six_steps, same_bits)

pytestmark = pytest.mark.gpu

NETS = FEATURE_NETS
BATCHES = (64, 128, 256)
FORMS = (("shuffled", (1, 2, 3, 5)), ("offset", (4,)), ("stored", (1, 2, 3, 5)))
TWIN_CASES = [(net, B, form, nb) for net in NETS for B in BATCHES for form, nbs in FORMS for nb in nbs]


def _data(spec, B):
    """5 x 256 rows whatever the batch, one draw per net"""
    return 5 * 256, 31000 + spec["F"]


# a single-GPU context (new step top) and a data-parallel context at a group of one (old)
pairs = cached_pairs(lambda net: Pair(NETS[net], F32, (("single", {}), ("dp", DP_GROUP_OF_ONE)), _data, path=5, resident=True), dp_group_of_one=True)


@pytest.mark.parametrize("net,B,form,nb", TWIN_CASES, ids=[f"{n}-B{b}-{f}-{k}steps" for n, b, f, k in TWIN_CASES])
def test_new_step_top_computes_the_old_step_top_s_bits(pairs, net, B, form, nb):
    twin = pairs(net)
    want = twin.run("dp", B, form, nb)
    got = twin.run("single", B, form, nb)
    print(net, B, form, nb, "costs", got[1].tolist())
    same_bits(got, want, twin.bits, "new step top against old")


ORACLE_CASES = [("784-30-10", [30], 100, 0), ("784-30-10", [30], 200, 0), ("784-10-10-10", [10, 10], 256, 0), ("784-10-10-10", [10, 10], 100, 0),
                ("784-30-10-gather", [30], 256, 1)]


@pytest.mark.parametrize("name,hidden,B,gather", ORACLE_CASES, ids=[f"{n}-B{b}" for n, _, b, _ in ORACLE_CASES])
def test_forms_without_an_old_top_twin_are_the_reference_loop(oracle, name, hidden, B, gather):
    from mercer_research_amd.device import DeviceRCN
    nb = 6
    X, Y, perm, ws, bs = one_and_six_inputs(hidden, 4100 + B + len(hidden), F32)
    d = DeviceRCN(dtype=F32, feedforward_cfg=hidden)
    d.set_dense_path(5)                                  # the resident kernel or an error: no other path can answer
    d.set_option("xcd_gather", gather)
    assert d.train_epoch_resident(B) and d.train_epoch_gathers(B) == bool(gather)
    got = one_and_six_steps(d, ws, bs, d.to_device(X, d.tdtype), d.to_device(Y, d.tdtype), d.to_device(perm), B, nb, runs=2)
    d.rcn.close()
    check_one_and_six(oracle, {name: got}, ws, bs, X, Y, perm, B, nb, F32_ONE_STEP, F32_SIX_STEPS)
