"""The feature worker's half of the resident one-XCD kernel's step in the single-GPU f32 forms for 64 samples and more: delta_1 of the
batch staged into LDS by loads that write LDS directly, in a lane-linear image whose odd sample rows have their two hidden halves
exchanged (csrc/dense_xcd.hpp: kD1Dma, xcd_d1_src_chunk / xcd_d1_word).  The results must be what they were.

Bit equality, new code against old.  The data-parallel form keeps the old staging (registers, rows of 48 floats), and at a group of ONE
rank its exchange adds nothing: the gathered sum is the rank's own partial.  So the single-GPU form must give the data-parallel form's
parameters and per-step costs as bits (set up as tests/test_gpu_resident_step_top.py: bootstrap over RCCL forced on).

The cases are chosen for what the staging and a transposed W_0 image can get wrong:
    batches 64, 128, 256       one, two and four 1 KB pieces per wave
    steps 1, 2, 3, 5           both batch-buffer parities, the image staged again over the last step's
    shuffled, offset, stored   a shuffled index, the same index entered one batch in, no index
    hidden 16, 17, 30, 32 at F = 36   the second hidden half of delta_1 and of the W_0 image all padding, one unit, masked, full --
                               the half the swizzle exchanges
    F =  36 -> NA =  2         the second worker has one slice with 4 live features
    F = 288 -> NA =  9         F = 784 -> NA = 25, the bench's net         F = 928 -> NA = 29, the largest
    classes 10 and 16
5 x 256 rows per net.

Oracle tolerance where no twin exists: the padded batches 100 and 200, the two-hidden-layer net 784-10-10-10 at 256 and 100 samples
and the gather form at 256 -- one step and six chained steps at the project's F32_ONE_STEP / F32_SIX_STEPS, two runs equal as bits.

Every case asserts that the resident kernel is what answers and that nothing stepped down.  Nothing here sets a fault option.
"""
import pytest
from _rcn_util import (DP_GROUP_OF_ONE, F32, F32_ONE_STEP, F32_SIX_STEPS, Pair, cached_pairs, check_one_and_six, feature_net, one_and_six_inputs,
                       one_and_six_steps, same_bits)

pytestmark = pytest.mark.gpu


def _net(shape, convpool, F, hidden=30, classes=10):
    return feature_net(shape, convpool, F, hidden, classes, NA=-(-(-(-F // 16)) // 2))


# one convolve + pool pair gives (h / 2) (w / 2) 4 features, the default two pairs (h / 4) (w / 4) 16
NETS = {"36-30-10": _net((6, 6), "one", 36), "36-16-10": _net((6, 6), "one", 36, hidden=16), "36-17-10": _net((6, 6), "one", 36, hidden=17),
        "36-32-10": _net((6, 6), "one", 36, hidden=32), "36-30-16": _net((6, 6), "one", 36, classes=16),
        "288-30-10": _net((16, 18), "one", 288), "784-30-10": _net((28, 28), "default", 784), "928-30-10": _net((16, 58), "one", 928),
        "784-30-16": _net((28, 28), "default", 784, classes=16)}
WANT_NA = {"36-30-10": 2, "288-30-10": 9, "784-30-10": 25, "928-30-10": 29}
BATCHES = (64, 128, 256)
FORMS = (("shuffled", (1, 2, 3, 5)), ("offset", (4,)), ("stored", (1, 2, 3, 5)))
TWIN_CASES = [(net, B, form, nb) for net in NETS for B in BATCHES for form, nbs in FORMS for nb in nbs]


def test_the_nets_cover_the_feature_worker_counts():
    for net, na in WANT_NA.items():
        assert NETS[net]["NA"] == na, (net, NETS[net]["NA"])


def _data(spec, B):
    """5 x 256 rows whatever the batch, one draw per net"""
    return 5 * 256, 61000 + spec["F"] + 7 * spec["hidden"] + spec["classes"]


def _twin(net):
    """a single-GPU context (new feature-worker code) and a data-parallel context at a group of one (old)"""
    twin = Pair(NETS[net], F32, (("single", {}), ("dp", DP_GROUP_OF_ONE)), _data, path=5, resident=True)
    for d in twin.ctx.values():
        assert -(-(-(-d.F // 16)) // 2) == NETS[net]["NA"], "the feature worker count this net is here for"
    return twin


pairs = cached_pairs(_twin, dp_group_of_one=True)


@pytest.mark.parametrize("net,B,form,nb", TWIN_CASES, ids=[f"{n}-B{b}-{f}-{k}steps" for n, b, f, k in TWIN_CASES])
def test_new_feature_worker_computes_the_old_one_s_bits(pairs, net, B, form, nb):
    twin = pairs(net)
    want = twin.run("dp", B, form, nb)
    got = twin.run("single", B, form, nb)
    print(net, "NA", NETS[net]["NA"], B, form, nb, "costs", got[1].tolist())
    same_bits(got, want, twin.bits, "new feature worker against old")


ORACLE_CASES = [("784-30-10", [30], 100, 0), ("784-30-10", [30], 200, 0), ("784-10-10-10", [10, 10], 256, 0), ("784-10-10-10", [10, 10], 100, 0),
                ("784-30-10-gather", [30], 256, 1)]


@pytest.mark.parametrize("name,hidden,B,gather", ORACLE_CASES, ids=[f"{n}-B{b}" for n, _, b, _ in ORACLE_CASES])
def test_forms_without_a_twin_are_the_reference_loop(oracle, name, hidden, B, gather):
    from mercer_research_amd.device import DeviceRCN
    nb = 6
    X, Y, perm, ws, bs = one_and_six_inputs(hidden, 6100 + B + len(hidden), F32)
    d = DeviceRCN(dtype=F32, feedforward_cfg=hidden)
    d.set_dense_path(5)                                  # the resident kernel or an error: no other path can answer
    d.set_option("xcd_gather", gather)
    assert d.train_epoch_resident(B) and d.train_epoch_gathers(B) == bool(gather)
    got = one_and_six_steps(d, ws, bs, d.to_device(X, d.tdtype), d.to_device(Y, d.tdtype), d.to_device(perm), B, nb, runs=2)
    d.rcn.close()
    check_one_and_six(oracle, {name: got}, ws, bs, X, Y, perm, B, nb, F32_ONE_STEP, F32_SIX_STEPS, costs_positive=True)
