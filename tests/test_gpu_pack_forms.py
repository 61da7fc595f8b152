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
import pytest
from _rcn_util import F32, F64, FEATURE_NETS, Pair, cached_pairs, feature_net, same_bits

pytestmark = pytest.mark.gpu

NETS = dict(FEATURE_NETS, **{"100-30-10": feature_net((10, 10), "one", 100)})
NETS.update({f"{net}/unaligned": dict(NETS[net], unaligned=True) for net in ("784-30-10", "36-30-10")})
DTYPES = {"f32": F32, "f64": F64}
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


def _data(spec, B):
    """five batches, a draw per net and batch size"""
    return 5 * B, 20250 + spec["F"] + B


def _pair(net, dtype, forms=(("parent", {"pack_form": 0}), ("rows", {"pack_form": 1})), path=None):
    """one net in one dtype: a context per pack form, on the path the library selects unless one is given"""
    return Pair(NETS[net], DTYPES[dtype], forms, _data, path=path)


pairs = cached_pairs(_pair)


@pytest.mark.parametrize("net,dtype,B,form,what", CASES, ids=[f"{n}-{t}-B{b}-{f}-{w}" for n, t, b, f, w in CASES])
def test_pack_rows_writes_the_image_of_pack_epoch(pairs, net, dtype, B, form, what):
    pair = pairs(net, dtype)
    want = pair.run("parent", B, form, what)
    got = pair.run("rows", B, form, what)
    print(net, dtype, B, form, what, "resident", pair.ctx["rows"].train_epoch_resident(B), "costs", got[1].tolist())
    same_bits(got, want, pair.bits, "pack_form 1 against 0")
    if what == "begin":                                  # ... and the begun epoch walked in two pieces is train_epoch over the same three batches
        same_bits(got, pair.run("rows", B, form, "3steps"), pair.bits, "epoch_begin + epoch_steps against train_epoch")


def test_pack_rows_image_gives_the_gather_form_s_bits(pairs):
    """pack_form = 1 against the resident kernel fetching its rows itself: no pack kernel on that side, so this does not rest on k_pack_epoch"""
    B = 256
    pair = pairs("784-30-10", "f32", forms=(("rows", {"pack_form": 1, "xcd_gather": 0}), ("gather", {"pack_form": 1, "xcd_gather": 1})), path=5)
    for name, gathers in (("rows", False), ("gather", True)):
        assert pair.ctx[name].train_epoch_resident(B) and pair.ctx[name].train_epoch_gathers(B) == gathers
    want = pair.run("gather", B, "shuffled", "3steps")
    got = pair.run("rows", B, "shuffled", "3steps")
    print("costs", got[1].tolist())
    same_bits(got, want, pair.bits, "packed image against the gather form")
