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
import pytest
from _rcn_util import F32, FEATURE_NETS, Pair, cached_pairs, same_bits

pytestmark = pytest.mark.gpu

B = 256
NETS = FEATURE_NETS
CASES = [(net, form, nb) for net in NETS for form, nbs in (("shuffled", (1, 2, 3, 5)), ("offset", (4,)), ("stored", (1, 2, 3, 5))) for nb in nbs]
GATHERS = {"packed": 0, "gather": 1}


def _data(spec, B):
    return 5 * B, 20250 + spec["F"]


# a context per form, on the resident kernel or an error: no other path can answer
pairs = cached_pairs(lambda net: Pair(NETS[net], F32, tuple((name, {"xcd_gather": opt}) for name, opt in GATHERS.items()), _data, path=5, resident=True))


@pytest.mark.parametrize("net,form,nb", CASES, ids=[f"{n}-{f}-{k}steps" for n, f, k in CASES])
def test_gather_form_computes_the_packed_form_s_bits(pairs, net, form, nb):
    pair = pairs(net)
    for name, opt in GATHERS.items():
        assert pair.ctx[name].train_epoch_gathers(B) == bool(opt)
    want = pair.run("packed", B, form, nb)
    got = pair.run("gather", B, form, nb)
    print(net, form, nb, "costs", got[1].tolist())
    same_bits(got, want, pair.bits, "gather form against packed")
