"""Batch normalisation without a GPU: the plans of the four BN nets (the launches per bn_relu layer, epilogue-1 convolutions, no conv+pool
fusion across a BN layer, who gates, one reduce job per BN layer), the state layout of the K = 1 block, the refusals, and the float64
torch helper of the GPU tests pinned on a case worked out by hand."""
import numpy as np
import pytest
from _torch_ref import TorchNet, n_logical, param_shapes, tensor_slices
from _convnet_util import convnet_loaded, plan_lines  # noqa: F401  (fixture)

# the nets of tests/test_gpu_convnet_bn.py: (input shape, layers, batch)
BN_A = ((8, 8, 3), (("conv_linear", 32), ("bn_relu",), ("pool",), ("conv_linear", 64), ("bn_relu",), ("pool",), ("dense_relu", 32), ("dense", 10)), 5)
BN_B = ((6, 6, 1), (("conv_linear", 32), ("bn_relu",), ("conv", 32), ("pool",), ("dense", 7)), 3)
BN_C = ((4, 4, 3), (("conv_linear", 32), ("bn_relu",), ("dense", 6)), 2)
BN_D = ((16, 16, 3), (("conv_linear", 32), ("bn_relu",), ("pool",), ("conv_linear", 64), ("bn_relu",), ("pool",), ("dense_relu", 128), ("dense", 10)), 64)
BN_NETS = {"a": BN_A, "b": BN_B, "c": BN_C, "d": BN_D}
# who gates each bn_relu layer's gradient, in the order of the BACKWARD walk (last BN layer first)
GATES = {"a": ["gated by the pool's backward"] * 2, "b": ["gated by the convolution above"], "c": ["gates itself (out > 0)"], "d": ["gated by the pool's backward"] * 2}


def _tags(lines):
    return [l.split(":")[0].split()[0] for l in lines]


@pytest.mark.parametrize("precision", ["fp32", "bf16"])
@pytest.mark.parametrize("name", sorted(BN_NETS))
def test_training_plan_names_the_bn_launches(convnet, name, precision):
    in_shape, layers, B = BN_NETS[name]
    lines = plan_lines(convnet.plan(in_shape, layers, B, precision))
    n_bn = sum(l[0] == "bn_relu" for l in layers)
    tags = _tags(lines)
    # forward: every bn-stats line is directly behind an epilogue-1 3x3 convolution and directly in front of its bn-relu line
    stats = [i for i, t in enumerate(tags) if t == "bn-stats"]
    assert len(stats) == n_bn
    for i in stats:
        assert lines[i - 1].startswith("conv3x3") and " epi 1:" in lines[i - 1] and "k_conv" in lines[i - 1], lines[i - 1]
        assert tags[i + 1] == "bn-relu" and "k_bn_apply_relu," in lines[i + 1], lines[i + 1]
        assert "k_bn_stats," in lines[i] and "k_bn_stats_finish" in lines[i]
    # backward: bn-bwd-reduce then bn-bwd-dx, once per layer, behind all the forward launches, with the right gate
    red = [i for i, t in enumerate(tags) if t == "bn-bwd-reduce"]
    assert len(red) == n_bn and min(red) > max(stats)
    for i, gate in zip(red, GATES[name]):
        assert tags[i + 1] == "bn-bwd-dx" and "k_bn_bwd_dx" in lines[i + 1], lines[i + 1]
        assert "k_bn_bwd_reduce" in lines[i] and "k_bn_bwd_finish" in lines[i] and lines[i].endswith(gate), lines[i]
    # the four launches of a layer in order: stats, relu ... reduce, dx
    order = [t for t in tags if t.startswith("bn-")]
    assert order == ["bn-stats", "bn-relu"] * n_bn + ["bn-bwd-reduce", "bn-bwd-dx"] * n_bn
    # no conv+pool fusion across a BN layer: a pool behind a bn_relu layer is k_pool_fwd / k_pool_bwd
    bn_at = [li for li, l in enumerate(layers) if l[0] == "bn_relu"]
    for i, li in zip(stats, bn_at):
        if layers[li + 1][0] == "pool":
            assert lines[i + 2].startswith("pool ") and lines[i + 2].endswith("k_pool_fwd"), lines[i + 2]
    for i, li in zip(red, reversed(bn_at)):
        if layers[li + 1][0] == "pool":
            assert lines[i - 1].startswith("pool-bwd") and lines[i - 1].endswith("k_pool_bwd"), lines[i - 1]
    # net b: the convolution above the BN layer gates with its output (epilogue 3); nets a, c, d have no epilogue-3 3x3 launch
    assert any(x.startswith("conv3x3") and " epi 3" in x for x in lines) == (name == "b")
    # no k_relu_bwd anywhere: a conv_linear layer has no gate of its own
    assert not any("k_relu_bwd" in x for x in lines)
    # one reduce job per layer with parameters, the BN layers among them
    n_par = sum(l[0] != "pool" for l in layers)
    assert lines[-1].startswith("update: k_reduce_all,") and f" {n_par} layers' slabs in one launch" in lines[-1], lines[-1]


@pytest.mark.parametrize("name", sorted(BN_NETS))
def test_eval_plan_shows_scale_and_shift(convnet, name):
    in_shape, layers, B = BN_NETS[name]
    lines = plan_lines(convnet.plan_eval(in_shape, layers, B))
    bn = [x for x in lines if x.startswith("bn-")]
    assert len(bn) == sum(l[0] == "bn_relu" for l in layers)
    assert all(x.startswith("bn-relu") and "k_bn_apply_relu<eval>" in x and "scale and shift from the running statistics" in x for x in bn), bn
    assert not any("bn-stats" in x for x in lines)


def test_first_layer_of_one_or_three_channels_gets_a_kernel(convnet):
    for name in "abcd":
        in_shape, layers, B = BN_NETS[name]
        for tiling in ("gemm", "auto", "lds"):
            first = plan_lines(convnet.plan(in_shape, layers, B, "fp32", tiling))[0]
            assert first.startswith(f"conv3x3 {in_shape[0]}x{in_shape[1]}x{in_shape[2]}->32 epi 1: k_conv"), first


def test_bucket_plan_walks_the_bn_layers(convnet):
    in_shape, layers, B = BN_A
    text = convnet.plan(in_shape, layers, B, buckets=0)
    assert text.count("bn-bwd-reduce") == 2 and text.count("bn-bwd-dx") == 2
    assert text.count("bucket") // 2 >= 6                     # six layers with parameters, one bucket each at min_bytes = 0


def test_state_layout_of_a_bn_net(convnet):
    in_shape, layers, _ = BN_A
    d = convnet.state_layout(in_shape, layers)
    sl = tensor_slices(in_shape, layers)
    assert d.n_log == n_logical(in_shape, layers) == sum((k + 1) * c for k, c in param_shapes(in_shape, layers))
    with_params = [i for i, l in enumerate(layers) if l[0] != "pool"]
    for (ws, _), li in zip(sl, with_params):
        assert d.layer_off[li] == ws.start, (li, d.layer_off[li], ws.start)
    # the BN layers: layer_off is the offset of gamma, and the block is 2 C long
    assert d.layer_off[1] == 27 * 32 + 32 and d.layer_off[3] - d.layer_off[1] == 2 * 32
    assert d.layer_off[4] == d.layer_off[3] + 9 * 32 * 64 + 64 and d.layer_off[6] - d.layer_off[4] == 2 * 64
    assert [d.layers[i].kind for i in range(d.n_layers)] == [convnet.KIND[l[0]] for l in layers]
    assert d.shape_and_layers()[1][1] == ("bn_relu",)
    # the same description without BN is 2 C per BN layer shorter
    plain = tuple(("conv", l[1]) if l[0] == "conv_linear" else l for l in layers if l[0] != "bn_relu")
    assert d.n_log - convnet.state_layout(in_shape, plain).n_log == 2 * 32 + 2 * 64


def test_bf16_stored_is_refused_with_a_reason(convnet):
    in_shape, layers, B = BN_A
    for fn in (convnet.plan, convnet.plan_eval):
        with pytest.raises(convnet.ConvNetError, match=r"-3: .*batch normalisation"):
            fn(in_shape, layers, B, "bf16_stored")


@pytest.mark.parametrize("layers", [
    (("conv", 32), ("bn_relu",), ("dense", 4)),                       # behind a ReLU convolution
    (("bn_relu",), ("dense", 4)),                                     # first
    (("conv_linear", 32), ("pool",), ("bn_relu",), ("dense", 4)),     # behind a pool
    (("conv_linear", 32), ("bn_relu",), ("bn_relu",), ("dense", 4)),  # behind another
])
def test_bn_not_behind_conv_linear_is_refused(convnet, layers):
    with pytest.raises(convnet.ConvNetError, match=r"-2: "):
        convnet.plan((4, 4, 32), layers, 2)


def test_conv_linear_without_bn_is_refused(convnet):
    with pytest.raises(convnet.ConvNetError, match=r"-2: .*RCN_HIPX_BN_RELU"):
        convnet.plan((4, 4, 32), (("conv_linear", 32), ("dense", 4)), 2)


def test_partial_sum_buffer_holds_every_smaller_batch(convnet):
    """The number of partials is NOT monotonic in the rows: 64 rows per partial up to 32768 rows (512 partials), 128 just above (257).  A
    layer's buffer is sized once for the net's largest batch, and a smaller batch -- the last one of an epoch -- may need more partials
    than the largest does: the capacity must cover every row count below it."""
    assert convnet.bn_partials(32768)[0] == 512 and convnet.bn_partials(33 * 1024)[0] == 264 and convnet.bn_partials(40 * 1024)[0] == 320
    assert convnet.bn_partials(33 * 1024)[1] == 512 and convnet.bn_partials(40 * 1024)[1] == 512
    rows = sorted(set(list(range(1, 2100)) + [k * 64 + d for k in (511, 512, 513, 1023, 1024, 1025, 2048, 8192) for d in (-1, 0, 1)] + [524288, 524289, 10 ** 7]))
    worst = 0                                             # the most partials of any row count so far
    for m in rows:
        parts, cap = convnet.bn_partials(m)
        assert 1 <= parts <= 512 and parts * ((m + parts - 1) // parts) >= m, (m, parts)
        worst = max(worst, parts)
        assert cap >= worst, (m, parts, cap, worst)       # (the capacity is monotonic, so this covers the row counts in between too)
        assert cap >= convnet.bn_partials(max(1, m - 63))[0] and cap <= 512
    caps = [convnet.bn_partials(m)[1] for m in rows]
    assert caps == sorted(caps)
    with pytest.raises(convnet.ConvNetError):
        convnet.bn_partials(0)


def test_plans_without_the_new_kinds_do_not_mention_bn(convnet):
    text = convnet.plan((8, 8, 3), (("conv", 32), ("pool",), ("dense", 10)), 4) + convnet.plan_eval((8, 8, 3), (("conv", 32), ("pool",), ("dense", 10)), 4)
    assert "bn" not in text


def test_bn_ref_on_a_hand_computed_case():
    """One pixel row of two channels through Conv2d -> BatchNorm2d -> ReLU, worked out by hand.  Input (1, 2, 1), B = 2; the 3x3 filter
    has only its centre tap, weights (2, -1) for the one input channel, biases (0, 1): x_conv[n, 0, w] = (2 v, -v + 1).
    v = [[1, 3], [5, 7]] (batch, width): channel 0 = 2, 6, 10, 14 -> mean 8, biased var 20; channel 1 = 0, -2, -4, -6 -> mean -3, var 5.
    gamma = (1, 2), beta = (0, 1), eps = 0.25: invstd = 1 / sqrt(20.25) = 1 / 4.5 and 1 / sqrt(5.25).
    A 32-channel minimum does not apply to the helper: it takes any description."""
    layers = (("conv_linear", 2), ("bn_relu",), ("dense", 1))
    w = np.zeros((9, 2)); w[4] = (2.0, -1.0)
    dense = np.array([1.0, 1.0, 1.0, 1.0])                  # sums the 2 x 2 features (w, c)
    flat = np.concatenate([w.ravel(), [0.0, 1.0], [1.0, 2.0], [0.0, 1.0], dense, [0.0]])
    net = TorchNet((1, 2, 1), layers, flat, momentum=0.5, eps=0.25)
    x = np.array([[1.0, 3.0], [5.0, 7.0]]).reshape(2, 1, 2, 1)
    z = net.logits(x, train=True)
    c0 = (np.array([2.0, 6.0, 10.0, 14.0]) - 8.0) / 4.5
    c1 = (np.array([0.0, -2.0, -4.0, -6.0]) + 3.0) / np.sqrt(5.25) * 2.0 + 1.0
    y = np.maximum(0.0, np.stack([c0, c1], axis=1)).reshape(2, 2, 2)          # (n, w, c)
    assert np.allclose(z.ravel(), y.sum(axis=(1, 2)), rtol=0, atol=1e-12), (z, y)
    # running statistics: r <- 0.5 r + 0.5 s from (0, 1), with the unbiased variance var * 4 / 3
    assert np.allclose(net.bn_stats(), [4.0, -1.5, 0.5 + 0.5 * 20 * 4 / 3, 0.5 + 0.5 * 5 * 4 / 3], rtol=0, atol=1e-12), net.bn_stats()
    # evaluation uses them
    ze = net.logits(x, train=False)
    rm, rv = net.bn_stats()[:2], net.bn_stats()[2:]
    xc = np.stack([[2.0, 6.0, 10.0, 14.0], [0.0, -2.0, -4.0, -6.0]], axis=1)
    ye = np.maximum(0.0, (xc - rm) / np.sqrt(rv + 0.25) * [1.0, 2.0] + [0.0, 1.0]).reshape(2, 2, 2)
    assert np.allclose(ze.ravel(), ye.sum(axis=(1, 2)), rtol=0, atol=1e-12), (ze, ye)
    # the flat views give back what went in, in the library's layout
    assert np.array_equal(net.params(), flat)
