"""GPU tests of the forms of Track X's stride-2, 1x1 and depthwise kernels that the three kind files leave unlaunched (the table and its
reasons: tests/_kinds_cases.py; that each case reaches its form, from the plan: tests/test_convnet_kinds_forms_plan.py): k_dw on bands of
16 and 32 rows at 1024 tiles, two slabs per row -- two bands with a seam, one band taller than the map, a channel quad that changes from
tile to tile -- and the same band forms on one-slab maps; k_pw with
3, 5, 6 and 7 accumulator tiles, K-tile counts that are no power of two and the [512][32] / [1024][32] slices of the LDS limit, with the
fall-back to the implicit GEMM one width further; the downsampling bottleneck and the separable downsampling block (a 1x1 and a depthwise
input gradient in front of k_skip_bwd_add_down); 2 x 2 -> 1 x 1, 1 x 1, H = 1 and W = 1 maps.  Every net runs tests/_twin_checks.py's
schedule -- a gradients call, two plain SGD steps, a forward and an evaluation on the running statistics -- against PyTorch on the CPU in
float64 (tests/_dw_ref.py's DwNet) at the stride tests' bounds (fp32 2e-4 of a tensor's scale + 1e-6, 4e-4 after a second step; bf16
operands 5e-3 / 2e-2 against the twin with the same operand rounding), no tensor widened.  Two of the tall-band nets run once more as
small-integer nets whose forward logits are NumPy's int64 bit for bit in both precisions; the two cross-kind blocks are held bit for bit
between twins, under set_overlap(1) and in buckets of one layer."""
import functools

import numpy as np
import pytest
from _convnet_util import LR, batches, dev, make_net, same_bits, step, twins
from _dw_ref import RTOL, RTOL_2, STEPS, compare, exact_case
from _kinds_cases import EXACT, EXACT_RUNS, NETS, PW0, PW1, RUNS, case, run_id, twin
from _twin_checks import device_run, grads, twin_schedule

pytestmark = pytest.mark.gpu


@functools.lru_cache(maxsize=None)
def _reference(name, precision):
    """the twin's side of a case, once for all its runs; nothing changes it"""
    flat, x, y = case(name)
    return twin_schedule(twin(name, precision, flat), x, y, STEPS)


@pytest.mark.parametrize("run", RUNS, ids=[run_id(r) for r in RUNS])
def test_schedule_against_the_float64_twin(run):
    name, precision, options = run
    flat, x, y = case(name)
    r = device_run(NETS[name], precision, flat, x, y, STEPS, options=tuple(options))
    compare(NETS[name], r, _reference(name, precision), RTOL[precision], RTOL_2[precision], STEPS, f"net {run_id(run)}")


# ---- exact data: two of the wide tall-band nets once more, where no tolerance comes in ---------------------------------------------------------

@functools.lru_cache(maxsize=None)
def _exact(name):
    return exact_case(spec=EXACT[name])


@pytest.mark.parametrize("name,options", EXACT_RUNS, ids=[f"{n}{'-looping' if o else ''}" for n, o in EXACT_RUNS])
def test_integer_nets_on_tall_bands_give_numpys_bits_in_both_precisions(name, options):
    """1024 tiles of 16 rows (two bands x two slabs, 24 quads: the quad changes between the slabs; on three looping workgroups on every
    tile) and of 32 rows (one band taller than the 28-row map x two slabs), forward"""
    import torch
    flat, stats, x, want, a2 = _exact(name)
    assert (a2 > 0).mean() > 0.2 and a2.max() <= 192 and np.abs(want).max() < 2 ** 24 and len(np.unique(want)) > 10
    for precision in ("fp32", "bf16"):
        net = make_net(EXACT[name], precision)
        for k, v in options:
            net.set_option(k, v)
        net.set_params(flat)
        net.set_bn_stats(stats)
        with torch.cuda.stream(net.stream):
            z = net.forward(dev(net, x))
        net.synchronize()
        z = z.cpu().numpy()
        net.close()
        assert same_bits(z, want.astype(np.float32)), (name, precision, np.abs(z - want).max())


# ---- the cross-kind blocks held bit for bit --------------------------------------------------------------------------------------------------

BLOCKS = [("neck", PW1), ("neck", PW0), ("sepdown", ())]
BLOCK_IDS = ["neck-k_pw", "neck-implicit-gemm", "sepdown"]


def _state(net):
    return net.get_params(), net.get_bn_stats(), net.get_velocity()


def _same(a, b):
    return all(same_bits(u, v) for u, v in zip(a, b))


def _twins(name, options, precision, count, **kw):
    """_convnet_util.twins with the block's options, and the plan's word that the launches the test is about run"""
    spec = NETS[name]
    nets = twins(spec, precision, count, **kw)
    for n in nets:
        for k, v in options:
            n.set_option(k, v)
        text = n.plan_of_this_net(spec[2])
        assert "k_skip_bwd_add_down" in text and ("k_pw<" in text) == (options == PW1) and ("k_dw<3>" in text) == (name == "sepdown"), text
    return nets


@pytest.mark.parametrize("precision", ["fp32", "bf16"])
@pytest.mark.parametrize("name,options", BLOCKS, ids=BLOCK_IDS)
def test_twins_are_bit_identical_over_three_momentum_steps(name, options, precision):
    a, b = _twins(name, options, precision, 2, sgd=(0.9, 0.0, False))
    for x, y in batches(a, NETS[name], 3):
        step(a, x, y, LR)
        step(b, x, y, LR)
    assert _same(_state(a), _state(b)) and a.get_velocity().any()
    a.close(), b.close()


@pytest.mark.parametrize("name,options", BLOCKS, ids=BLOCK_IDS)
def test_overlap_changes_no_bit(name, options):
    """the weight gradients on the second stream never read the source's gradient that the input gradient and k_skip_bwd_add_down write"""
    spec = NETS[name]
    a, b = _twins(name, options, "fp32", 2)
    b.set_overlap(1)
    x, y = batches(a, spec, 1)[0]
    ga, la, za = grads(a, x, y, spec[2])
    gb, lb, zb = grads(b, x, y, spec[2])
    assert same_bits(ga, gb) and la == lb and same_bits(za, zb)
    for _ in range(2):
        step(a, x, y, LR)
        step(b, x, y, LR)
    assert _same(_state(a), _state(b))
    a.close(), b.close()


@pytest.mark.parametrize("name,options", BLOCKS, ids=BLOCK_IDS)
def test_buckets_of_one_layer_change_no_bit(name, options):
    """at 0 bytes every layer is a bucket: one ends between the skip's add (in the iteration of the layer above the source) and the source"""
    import torch
    spec = NETS[name]
    net, = _twins(name, options, "fp32", 1)
    x, y = batches(net, spec, 1)[0]
    g, _, _ = grads(net, x, y, spec[2])
    gb = torch.zeros(net.n_padded, dtype=torch.float32, device=net.device)
    seen = []
    with torch.cuda.stream(net.stream):
        net.gradients_bucketed(x, y, gb, min_bucket_bytes=0, on_bucket=lambda *a: seen.append(a))
    net.synchronize()
    assert len(seen) > 2 and same_bits(net.unpad(gb), g)
    net.close()
