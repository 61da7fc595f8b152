"""Global average pooling without a GPU: ("global_avgpool",) = AdaptiveAvgPool2d(1) + flatten(1) in front of the dense stage
(include/rcn_hipx.h: RCN_HIPX_GLOBAL_AVGPOOL; csrc/convnet_gap.hpp).  The plans of the nets of tests/test_gpu_convnet_gap.py (the two
launches, who gates what), the head's K = C, every refusal of a description, the state layout, the float64 torch twin of the GPU tests
(tests/_torch_ref.py) pinned on a case worked out by hand, and the premises of the GPU file's exact, gate and count checks."""
import functools
from fractions import Fraction

import numpy as np
import pytest
from _convnet_util import convnet_loaded, plan_lines  # noqa: F401  (fixture)
from _gap_cases import exact_forward, exact_gate_case, exact_logit_case, im2col, rows_seen
from _torch_ref import TorchNet, n_logical, param_shapes, random_params, tensor_slices
from _twin_checks import twin_schedule

# (input shape, layers, batch): the smallest nets at which each path of the two kernels can go wrong
# a: a ReLU convolution below: gated by the pool, no k_relu_bwd; HW = 16
GAP_A = ((4, 4, 3), (("conv", 32), ("global_avgpool",), ("dense", 10)), 3)
GAP_A1 = (GAP_A[0], GAP_A[1], 1)
# b: bn_add_relu below: batch normalisation and the skip take their "gated above" forms; HW = 16; a dropout site behind the pool
GAP_B = ((8, 8, 3), (("conv", 32), ("pool",), ("conv_linear", 32), ("bn_relu",), ("conv_linear", 32), ("bn_add_relu", 4), ("global_avgpool",),
                     ("dense_relu", 32), ("dense", 10)), 4)
# c: a max-pool below: ungated; HW = 36 (an inexact division), C = 96 (24 columns x 10 slices, 16 threads idle)
GAP_C = ((12, 12, 3), (("conv", 96), ("pool",), ("global_avgpool",), ("dense", 5)), 3)
# d: bn_relu below; HW = 196: more rows than the 16 slices of 16 columns, and no multiple of them
GAP_D = ((14, 14, 1), (("conv", 32), ("conv_linear", 64), ("bn_relu",), ("global_avgpool",), ("dense", 10)), 2)
# e: HW = 4: fewer rows than the 32 slices of 8 columns -- 28 slices hold no row
GAP_E = ((2, 2, 3), (("conv", 32), ("global_avgpool",), ("dense", 10)), 3)
# loop: net a at a batch whose map has more 16-byte pieces than the backward kernel's capped grid has threads: a second grid-stride trip
GAP_LOOP = (GAP_A[0], GAP_A[1], 8200)
GAP_NETS = {"a": GAP_A, "a1": GAP_A1, "b": GAP_B, "c": GAP_C, "d": GAP_D, "e": GAP_E}
# per net: (H, W, C of the pooled map, the layer below, gate words of gap-bwd)
GAP_LINES = {
    "a": (4, 4, 32, 0, "gated here with layer 0's output (out > 0)"),
    "a1": (4, 4, 32, 0, "gated here with layer 0's output (out > 0)"),
    "b": (4, 4, 32, 5, "gated here with layer 5's output (out > 0)"),
    "c": (6, 6, 96, 1, "ungated: layer 1 is a pool"),
    "d": (14, 14, 64, 2, "gated here with layer 2's output (out > 0)"),
    "e": (2, 2, 32, 0, "gated here with layer 0's output (out > 0)"),
}
ABOVE = "gated by the global average pool above"
RTOL = {"fp32": 2e-4, "bf16": 5e-3}                     # tests/test_gpu_convnet_res.py's bounds
RTOL_2 = {"fp32": 4e-4, "bf16": 2e-2}                   # ... after a second step
# the first seed per net at which the twin's evaluation logits keep twice the margin the count check needs, in both precisions
SEEDS = {"a": 1, "a1": 4, "b": 1, "c": 1, "d": 2, "e": 2}
STEPS = 2


def data(spec, seed):
    in_shape, layers, B = spec
    rng = np.random.default_rng(seed)
    flat = random_params(rng, in_shape, layers)
    x = rng.standard_normal((B,) + in_shape).astype(np.float32)
    y = rng.integers(0, layers[-1][1], B).astype(np.int32)
    return flat, x, y


@functools.lru_cache(maxsize=None)
def twin_run(name, precision):
    """What the float64 twin makes of the GPU file's run on net `name`: one gradients call, STEPS plain SGD steps, then a forward and an
    evaluation on the running statistics.  Computed once per process and shared by the CPU and GPU files."""
    spec = GAP_NETS[name]
    in_shape, layers, B = spec
    flat, x, y = data(spec, SEEDS[name])
    ref = TorchNet(in_shape, layers, flat, operand="bf16" if precision == "bf16" else "f64")
    return twin_schedule(ref, x, y, STEPS)


def _tags(lines):
    return [l.split(":")[0].split()[0] for l in lines]


def _workgroups(line):
    return int(line.split(" workgroups")[0].rsplit(" ", 1)[1])


# ---- plans ----------------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("precision", ["fp32", "bf16"])
@pytest.mark.parametrize("name", sorted(GAP_NETS))
def test_training_plan_names_the_two_launches_and_who_gates(convnet, name, precision):
    in_shape, layers, B = GAP_NETS[name]
    H, W, C, below, words = GAP_LINES[name]
    lines = plan_lines(convnet.plan(in_shape, layers, B, precision))
    tags = _tags(lines)
    assert tags.count("gap-fwd") == tags.count("gap-bwd") == 1
    fwd, bwd = lines[tags.index("gap-fwd")], lines[tags.index("gap-bwd")]
    col_blocks = -(-(C // 4) // 64)
    assert fwd == f"gap-fwd {H}x{W}x{C}: k_gap_fwd, {B * col_blocks} workgroups", fwd
    n4 = B * H * W * C // 4
    assert bwd.startswith(f"gap-bwd {H}x{W}x{C}: k_gap_bwd, ") and bwd.endswith(f" workgroups ({words})"), bwd
    assert _workgroups(bwd) >= -(-n4 // 256) and (_workgroups(bwd) * 256) % (C // 4) == 0, bwd
    # forward: directly in front of the first dense launch (K = C); backward: directly behind that layer's weight gradient
    gi = [l[0] for l in layers].index("global_avgpool")
    units = -(-layers[gi + 1][1] // 32) * 32
    assert lines[tags.index("gap-fwd") + 1].startswith(f"dense 1x1x{C}->{units} "), lines[tags.index("gap-fwd") + 1]
    assert lines[tags.index("gap-bwd") - 1].startswith(f"wgrad dense 1x1x{C}->{units}:"), lines[tags.index("gap-bwd") - 1]
    # the dense layer above writes the pool's gradient UNGATED (epilogue 0)
    assert lines[tags.index("gap-bwd") - 2].startswith(f"dense 1x1x{units}->{C} epi 0:"), lines[tags.index("gap-bwd") - 2]
    assert not any("k_relu_bwd" in l for l in lines), "the layer below the pool finds its dZ ready"
    assert below == gi - 1
    n_par = sum(l[0] not in ("pool", "global_avgpool") for l in layers)
    assert lines[-1].startswith("update: k_reduce_all,") and f" {n_par} layers' slabs in one launch" in lines[-1], lines[-1]


def test_the_layers_below_take_their_gated_forms(convnet):
    """net b: the bn_add_relu layer below the pool, and the skip it feeds, are "gated by the global average pool above"; the bn_relu layer
    further down still by the convolution above it.  net d: its bn_relu.  net c: the pool gates in its own backward."""
    lines = plan_lines(convnet.plan(*GAP_B))
    reduces = [l for l in lines if l.startswith("bn-bwd-reduce")]
    assert len(reduces) == 2 and reduces[0].endswith("; " + ABOVE) and reduces[1].endswith("; gated by the convolution above"), reduces
    skip, = [l for l in lines if l.startswith("skip-bwd")]
    assert f"(the skip's gradient {ABOVE}; ungated: layer 1 is a pool)" in skip, skip
    assert _tags(lines).index("gap-bwd") < _tags(lines).index("bn-bwd-reduce")
    reduces = [l for l in plan_lines(convnet.plan(*GAP_D)) if l.startswith("bn-bwd-reduce")]
    assert len(reduces) == 1 and reduces[0].endswith("; " + ABOVE), reduces
    for tiling, pool_line in (("auto", "pool-bwd 12x12x96: k_pool_bwd"), ("lds", "pool-bwd 12x12x96: none (the convolution's gradient kernels unpool while staging)")):
        lines = plan_lines(convnet.plan(*GAP_C, "fp32", tiling))
        assert lines[_tags(lines).index("gap-bwd") + 1] == pool_line, lines


@pytest.mark.parametrize("name", sorted(GAP_NETS))
def test_eval_plan_has_the_forward_launch_and_no_backward(convnet, name):
    in_shape, layers, B = GAP_NETS[name]
    ev = plan_lines(convnet.plan_eval(in_shape, layers, B))
    train = plan_lines(convnet.plan(in_shape, layers, B))
    fwd, = [l for l in ev if l.startswith("gap-fwd")]
    assert fwd in train and not any(l.startswith("gap-bwd") for l in ev)


def test_bucket_plan_puts_the_boundary_directly_above_the_pool(convnet):
    """A bucket ends with a layer that HAS parameters, so the pool always opens the bucket of the layer below it: at 0 bytes the dense
    layer above is a bucket of its own and the boundary lies directly above the pool; no boundary can lie directly below it."""
    for spec, gi in ((GAP_B, 6), (GAP_C, 2)):
        lines = [l.strip() for l in convnet.plan(*spec, buckets=0).splitlines()]
        i, = [k for k, x in enumerate(lines) if x.startswith("gap-bwd")]
        assert lines[i - 1].startswith("bucket") and lines[i - 1].endswith(f": layers {gi} .. {gi - 1 if spec is GAP_B else 0}"), lines[i - 1]
        assert " done: grad[" in lines[i - 2], lines[i - 2]


def test_loop_case_takes_a_second_grid_stride_trip(convnet):
    """k_gap_bwd's grid is capped at 4096 workgroups of 256 threads; the loop case has more pieces than that.  k_gap_fwd has no loop:
    one workgroup per sample and block of 64 columns, whatever B."""
    in_shape, layers, B = GAP_LOOP
    n4 = B * 16 * 32 // 4
    assert 4096 * 256 < n4 < 2 * 4096 * 256
    lines = plan_lines(convnet.plan(in_shape, layers, B))
    bwd, = [l for l in lines if l.startswith("gap-bwd")]
    fwd, = [l for l in lines if l.startswith("gap-fwd")]
    assert _workgroups(bwd) == 4096 and _workgroups(fwd) == B, (bwd, fwd)


def test_existing_nets_plans_do_not_name_the_layer(convnet):
    from bench_convnet import CONFIGS
    for name in ("cifar", "mnist", "cifar_bn", "cifar_res"):
        text = convnet.plan(*CONFIGS[name])
        assert "gap" not in text and "global average" not in text, name


def test_bench_config_ends_as_a_resnet_does(convnet):
    from bench_convnet import CONFIGS
    in_shape, layers, B = CONFIGS["cifar_res_gap"]
    res = CONFIGS["cifar_res"][1]
    assert layers[:-2] == res[:-3] and layers[-2:] == (("global_avgpool",), ("dense", 10)) and res[-3:] == (("pool",), ("dense_relu", 256), ("dense", 10))
    lines = plan_lines(convnet.plan(in_shape, layers, B))
    assert "gap-fwd 8x8x128: k_gap_fwd, 512 workgroups" in lines
    assert any(l.startswith("dense 1x1x128->32 ") for l in lines)
    assert param_shapes(in_shape, layers)[-1] == (128, 10)


# ---- shapes, parameters, state --------------------------------------------------------------------------------------------------------------

def test_param_count_shows_the_head_with_k_equal_c(convnet):
    for name, spec in GAP_NETS.items():
        in_shape, layers, _ = spec
        d = convnet.state_layout(in_shape, layers)
        assert d.n_log == n_logical(in_shape, layers), name
        gi = [l[0] for l in layers].index("global_avgpool")
        C = GAP_LINES[name][2]
        head = tensor_slices(in_shape, layers)[sum(l[0] not in ("pool", "global_avgpool") for l in layers[:gi])]      # the layer behind the pool
        assert head[0].stop - head[0].start == C * layers[gi + 1][1], name           # K = C, not H * W * C
    # the same description at another resolution has the same parameters
    assert convnet.state_layout((8, 8, 3), GAP_A[1]).n_log == convnet.state_layout((4, 4, 3), GAP_A[1]).n_log == 27 * 32 + 32 + 32 * 10 + 10


def test_state_layout_keeps_kind_7_out_0(convnet):
    in_shape, layers, _ = GAP_B
    d = convnet.state_layout(in_shape, layers)
    assert convnet.KIND["global_avgpool"] == 7 and d.version == 1
    assert [d.layers[i].kind for i in range(d.n_layers)] == [convnet.KIND[l[0]] for l in layers]
    assert (d.layers[6].kind, d.layers[6].out) == (7, 0) and d.layer_off[6] == -1 and d.layer_off[1] == -1
    assert (d.layers[5].kind, d.layers[5].out) == (6, 4)
    assert d.shape_and_layers() == (in_shape, [tuple(l) for l in layers])
    assert d.layer_off[7] == tensor_slices(in_shape, layers)[5][0].start
    body = np.zeros(int(d.body_bytes), dtype=np.uint8)
    d2, body2, extra = convnet.read_state_file(convnet.write_state_file(d, body, b"x"))
    assert d2.shape_and_layers() == (in_shape, [tuple(l) for l in layers]) and (d2.layers[6].kind, d2.layers[6].out) == (7, 0)
    assert extra == b"x" and body2.size == body.size


def test_hbm_floor_counts_the_pool(convnet):
    """forward: the map read, [B][C] written; backward: [B][C] read, the map's gradient written -- and the head shrinks to K = C"""
    floor = convnet.ConvNet.step_hbm_floor_bytes
    mk = lambda in_shape, layers: type("N", (), {"in_shape": in_shape, "layers": [tuple(l) for l in layers]})()
    B, i, m, o = 5, 4 * 4 * 3 * 4, 4 * 4 * 32 * 4, 32 * 4
    conv = B * 2 * (i + m) + 3 * (27 * 32 + 32) * 4                   # a first layer: no input gradient
    head = B * 3 * (o + 40) + 3 * (32 * 10 + 10) * 4                  # K = 32
    assert floor(mk(*GAP_A[:2]), B) == conv + B * 2 * (m + o) + head


REFUSALS = [
    # (layers on a 4 x 4 x 32 input, status, the message names)
    ((("global_avgpool",), ("dense", 4)), -2, r"layer 0 \(RCN_HIPX_GLOBAL_AVGPOOL\): .*first layer"),
    ((("conv", 32), ("dense_relu", 32), ("global_avgpool",), ("dense", 4)), -2, r"layer 2 \(RCN_HIPX_GLOBAL_AVGPOOL\): .*dense layer or another global average pool \(layer 1\)"),
    ((("conv", 32), ("global_avgpool",), ("global_avgpool",), ("dense", 4)), -2, r"layer 2 \(RCN_HIPX_GLOBAL_AVGPOOL\): .*dense layer or another global average pool \(layer 1\)"),
    ((("conv", 32), ("conv_linear", 32), ("global_avgpool",), ("dense", 4)), -2, r"layer 1: a RCN_HIPX_CONV3X3 layer must be followed by RCN_HIPX_BN_RELU or RCN_HIPX_BN_ADD_RELU"),
    # what may not follow a dense layer may not follow the pool: the `flat` messages name both
    ((("conv", 32), ("global_avgpool",), ("conv", 32), ("dense", 4)), -2, r"convolution after a dense layer or a global average pool"),
    ((("conv", 32), ("global_avgpool",), ("pool",), ("dense", 4)), -2, r"max-pool must follow a convolution"),
    ((("conv", 32), ("global_avgpool",), ("bn_relu",), ("dense", 4)), -2, r".*must directly follow a RCN_HIPX_CONV3X3 layer"),
    ((("conv", 32), ("global_avgpool",)), -2, r"the last layer must be RCN_HIPX_DENSE"),
]


@pytest.mark.parametrize("layers,status,message", REFUSALS, ids=[str(k) for k in range(len(REFUSALS))])
def test_refusals_return_their_status_and_name_the_layer(convnet, layers, status, message):
    for fn in (convnet.plan, convnet.plan_eval):
        with pytest.raises(convnet.ConvNetError, match=rf": {status}: {message}"):
            fn((4, 4, 32), layers, 2)
    with pytest.raises(convnet.ConvNetError, match=rf"rcn_hipx_state_layout: {status}$"):
        convnet.state_layout((4, 4, 32), layers)


def test_accepted_behind_each_of_the_four_kinds(convnet):
    for layers in ((("conv", 32), ("global_avgpool",), ("dense", 4)), (("conv_linear", 32), ("bn_relu",), ("global_avgpool",), ("dense", 4)),
                   (("conv", 32), ("conv_linear", 32), ("bn_relu",), ("conv_linear", 32), ("bn_add_relu", 4), ("global_avgpool",), ("dense", 4)),
                   (("conv", 32), ("pool",), ("global_avgpool",), ("dense_relu", 64), ("dense_relu", 32), ("dense", 4))):
        assert "gap-fwd" in convnet.plan((4, 4, 32), layers, 2)


def test_bf16_stored_is_refused_with_the_pools_reason(convnet):
    for spec in (GAP_A, GAP_B, GAP_C):
        for fn in (convnet.plan, convnet.plan_eval):
            with pytest.raises(convnet.ConvNetError, match=r"-3: .*RCN_HIPX_BF16_STORED.* does not cover global average pooling"):
                fn(*spec, "bf16_stored")


# ---- the twin -------------------------------------------------------------------------------------------------------------------------------

def test_gap_ref_on_a_hand_computed_case():
    """2 samples, a 2 x 2 map, 2 channels; the convolution is its centre tap = identity (bias 0), so the map below the pool is relu(x).
        sample 0: channel 0 = (1, 2, 3, 6) -> mean 3        channel 1 = (4, -8, 0.5, 1.5) -> relu (4, 0, 0.5, 1.5), mean 1.5: ONE closed ReLU
        sample 1: channel 0 = (2, 2, 2, 2) -> mean 2        channel 1 = (1, 3, 5, 7) -> mean 4
    dense 2 -> 1 with w = (2, -4), b = 0.5: z = (2 * 3 - 4 * 1.5 + 0.5, 2 * 2 - 4 * 4 + 0.5) = (0.5, -11.5); L = 1 z_0 + 3 z_1.
    dL/dmean[b][c] = v_b w_c, and every OPEN position of the map gets a quarter of it: (0.5, -1) for sample 0, (1.5, -3) for sample 1."""
    x = np.zeros((2, 2, 2, 2))
    x[0, :, :, 0], x[0, :, :, 1] = [[1, 2], [3, 6]], [[4, -8], [0.5, 1.5]]
    x[1, :, :, 0], x[1, :, :, 1] = [[2, 2], [2, 2]], [[1, 3], [5, 7]]
    eye = np.zeros((18, 2)); eye[8:10] = np.eye(2)
    layers = (("conv", 2), ("global_avgpool",), ("dense", 1))
    flat = np.concatenate([eye.ravel(), np.zeros(2), [2.0, -4.0], [0.5]])
    assert n_logical((2, 2, 2), layers) == flat.size and param_shapes((2, 2, 2), layers) == [(18, 2), (2, 1)]
    net = TorchNet((2, 2, 2), layers, flat)
    z = net.forward(x, True)
    assert np.array_equal(net.outs[1].detach().numpy(), [[3.0, 1.5], [2.0, 4.0]])
    assert np.array_equal(z.detach().numpy().ravel(), [0.5, -11.5])
    net.outs[0].retain_grad()
    (z[:, 0] * net.torch.tensor([1.0, 3.0], dtype=net.torch.float64)).sum().backward()
    got = net.outs[0].grad.numpy().transpose(0, 2, 3, 1)                 # NHWC
    want = np.zeros((2, 2, 2, 2))
    want[0, :, :, 0], want[0, :, :, 1] = 0.5, [[-1.0, -1.0], [-1.0, -1.0]]
    want[1, :, :, 0], want[1, :, :, 1] = 1.5, -3.0
    assert np.array_equal(got, want)
    # the gradient INTO the convolution's pre-activation is gated: the closed position gets nothing
    loose = TorchNet((2, 2, 2), layers, flat, gate_below=False)
    zl = loose.forward(x, True)
    assert np.array_equal(zl.detach().numpy(), z.detach().numpy())
    # the closed position is pixel (0, 1) of channel 1 of sample 0 (x = -8): the convolution's bias gradient counts it only without the gate

    def conv_bias_grad(n):
        for m in n.mods:
            m.zero_grad()
        (n.forward(x, True)[:, 0] * n.torch.tensor([1.0, 3.0], dtype=n.torch.float64)).sum().backward()
        return n.mods[0].bias.grad.numpy()
    assert np.array_equal(conv_bias_grad(TorchNet((2, 2, 2), layers, flat)), [4 * 0.5 + 4 * 1.5, 3 * -1.0 + 4 * -3.0])
    assert np.array_equal(conv_bias_grad(loose), [4 * 0.5 + 4 * 1.5, 4 * -1.0 + 4 * -3.0])
    assert np.array_equal(net.params(), flat)


@pytest.mark.parametrize("precision", ["fp32", "bf16"])
@pytest.mark.parametrize("name", sorted(GAP_NETS))
def test_the_twins_margin_makes_the_correct_count_exact(name, precision):
    """tests/test_gpu_convnet_gap.py compares the correct count whenever no row's two best evaluation logits are within reach of the
    tolerance: with these seeds the twin alone says that holds on every net, so that check always runs."""
    r = twin_run(name, precision)
    print(f"{name} {precision}: margin {r['margin']:.3e}, needed {4 * RTOL_2[precision] * r['scale']:.3e}")
    assert r["margin"] > 4 * RTOL_2[precision] * r["scale"], (r["margin"], r["scale"])


# ---- the premises of the exact tests --------------------------------------------------------------------------------------------------------

EXACT_SHAPES = {"a": ((4, 4, 3), 32, 10, 3), "e": ((2, 2, 3), 32, 10, 3)}      # in_shape, C, classes, B


@pytest.mark.parametrize("name", sorted(EXACT_SHAPES))
def test_exact_logit_case_is_exact_in_fp32(name):
    """Every map value is a positive integer below 2**6, so every partial sum of a column in ANY order is an integer below 2**24 (exact in
    fp32 and in double); HW is a power of two, so the division is exact; the means are multiples of 1 / HW, the dense weights of 1 / 4, and
    the sum of the absolute terms of every logit stays below 2**20 quanta of 1 / (4 HW).  One row left out, or counted twice, changes every
    channel's mean -- every value is at least 1."""
    in_shape, C, classes, B = EXACT_SHAPES[name]
    x, y, w0, b0, w1, b1, flat = exact_logit_case(in_shape, C, classes, B)
    assert np.array_equal(flat.astype(np.float64), np.concatenate([w0.ravel(), b0, w1.ravel(), b1]))
    a, m, z = exact_forward(x, w0, b0, w1, b1)
    HW = in_shape[0] * in_shape[1]
    assert HW & (HW - 1) == 0
    assert np.array_equal(a, np.rint(a)) and a.min() >= 1 and a.max() < 2 ** 6
    # exact rational arithmetic agrees with the float64 restatement, and float32 holds every value
    for b in range(B):
        for c in range(C):
            s = sum(Fraction(int(v)) for v in a[b, :, c])
            assert Fraction(float(m[b, c])) == s / HW and np.float32(m[b, c]) == m[b, c]
            for drop in range(HW):
                assert (s - int(a[b, drop, c])) / HW != s / HW and (s + int(a[b, drop, c])) / HW != s / HW
    q = 1.0 / (4 * HW)
    assert np.array_equal(m / (1.0 / HW), np.rint(m * HW)) and np.array_equal(w1 * 4, np.rint(w1 * 4)) and np.array_equal(b1 * 4, np.rint(b1 * 4))
    assert ((np.abs(m) @ np.abs(w1) + np.abs(b1)) / q).max() < 2 ** 20
    zf = [[sum(Fraction(float(m[b, c])) * Fraction(float(w1[c, j])) for c in range(C)) + Fraction(float(b1[j])) for j in range(classes)] for b in range(B)]
    assert all(Fraction(float(z[b, j])) == zf[b][j] for b in range(B) for j in range(classes))
    assert np.array_equal(z.astype(np.float32).astype(np.float64), z)
    assert len(np.unique(z)) > classes                                  # not a degenerate case


GATE_PIXELS = {"a": [(1, 1), (1, 2), (2, 1), (2, 2)], "e": [(0, 0)]}


@pytest.mark.parametrize("name", sorted(EXACT_SHAPES))
def test_exact_gate_case_shows_every_row_and_both_gate_states(name):
    """One sample, one non-zero input value: the map is a small integer everywhere (sums of at most two integers), the rows the pixel
    reaches cover the whole map over the case's pixels, both gate states occur among them, every dense row has one non-zero +-1 / 2 (the
    pool's gradient is a power of two times ONE d logit: exact), and the quotient by HW, a power of two, is exact."""
    in_shape, C, classes, _ = EXACT_SHAPES[name]
    HW = in_shape[0] * in_shape[1]
    seen, opened, shut = set(), 0, 0
    for k, pixel in enumerate(GATE_PIXELS[name]):
        x, y, w0, b0, w1, b1, flat = exact_gate_case(in_shape, C, classes, pixel, seed=k)
        assert np.array_equal(flat.astype(np.float64), np.concatenate([w0.ravel(), b0, w1.ravel(), b1]))
        a, m, z = exact_forward(x, w0, b0, w1, b1)
        assert np.array_equal(a, np.rint(a)) and a.max() <= 4 and np.array_equal(m * HW, np.rint(m * HW))
        assert ((w1 != 0).sum(1) == 1).all() and set(np.abs(w1[w1 != 0])) == {0.5}
        rows = rows_seen(in_shape, pixel)
        seen |= set(rows.values())
        opened += int((a[0, list(rows.values())] > 0).sum())
        shut += int((a[0, list(rows.values())] == 0).sum())
        # the patch column of (tap, channel 0) is the indicator of that one row
        cols = im2col(x.astype(np.float64))
        for tap, row in rows.items():
            assert cols[:, tap * in_shape[2]].tolist() == [1.0 if r == row else 0.0 for r in range(HW)]
    assert seen == set(range(HW)) and opened > 20 and shut > 20, (seen, opened, shut)


def gate_case():
    """net a on Gaussian data: about half of the convolution's pre-activations are negative"""
    return data(GAP_A, 13)


def test_gate_case_closes_between_a_fifth_and_four_fifths():
    """the data of the GPU file's gate test: net a, and the twin without the pool's gate is many allowances away from the true gradient"""
    flat, x, y = gate_case()
    in_shape, layers, _ = GAP_A
    ref = TorchNet(in_shape, layers, flat)
    _, _, g_true = ref.loss_and_grads(x, y)
    zero = float((ref.outs[0].detach().numpy() == 0).mean())
    print(f"{zero:.2f} of the convolution's output is zero")
    assert 0.2 <= zero <= 0.8, zero
    _, _, g_loose = TorchNet(in_shape, layers, flat, gate_below=False).loss_and_grads(x, y)
    worst = 0.0
    for ws, bs in tensor_slices(in_shape, layers)[:1]:
        for t in (ws, bs):
            worst = max(worst, float(np.abs(g_loose[t] - g_true[t]).max()) / (2e-4 * max(1e-3, float(np.abs(g_true[t]).max())) + 1e-6))
    print(f"no gate below the pool: worst |d| / allowance = {worst:.1f}")
    assert worst > 100.0, worst
