"""Residual blocks without a GPU: ("bn_add_relu", d) = relu(BatchNorm2d(z) + s), s the output of the layer d places in front
(include/rcn_hipx.h: RCN_HIPX_BN_ADD_RELU).  The plans of the four nets of tests/test_gpu_convnet_res.py (the apply launch with its skip,
the add pass of the backward walk directly behind the input-gradient launch of the layer above the source, who gates what), every refusal
of a description, the state layout, and the float64 torch twin of the GPU tests (tests/_torch_ref.py) pinned on a case worked out by hand."""
import numpy as np
import pytest
from _convnet_util import convnet_loaded, plan_lines  # noqa: F401  (fixture)
from _torch_ref import TorchNet, n_logical, plain, skips, tensor_slices


def block(c):
    """a basic block of width c behind the layer that made its input"""
    return (("conv_linear", c), ("bn_relu",), ("conv_linear", c), ("bn_add_relu", 4))


# (input shape, layers, batch): the smallest nets at which each path of the skip can go wrong
# a: the source is a ReLU convolution, gated by the input-gradient launch above it; the block's output is gated by the pool's backward
RES_A = ((8, 8, 3), (("conv", 32),) + block(32) + (("pool",), ("dense", 10)), 5)
# b: the source is a pool (ungated add; its gradient is then read by the convolution below the pool); the output is gated by the convolution above
RES_B = ((8, 8, 3), (("conv", 32), ("pool",)) + block(32) + (("conv", 32), ("pool",), ("dense", 7)), 3)
# c: source bn_relu, then source bn_add_relu (a gradient that itself receives a skip, and is gated); the last output gates itself; 32 rows
RES_C = ((4, 4, 3), (("conv_linear", 32), ("bn_relu",)) + block(32) + block(32) + (("dense", 6),), 2)
# d: 133120 rows: the streaming kernels' grid-stride loops take a second trip for some threads, the sums have 416 partials
RES_D = ((32, 32, 3), (("conv", 32),) + block(32) + (("pool",), ("dense", 10)), 130)
RES_NETS = {"a": RES_A, "b": RES_B, "c": RES_C, "d": RES_D}
SELF_POOL, SELF_CONV, SELF_HERE = "gated by the pool's backward", "gated by the convolution above", "gated here (out > 0)"
# per skip-bwd line in the order of the backward walk: (source S, the skip's own gate, the source's gate, bn-bwd-reduce lines in front of it
# = the batch-normalisation layers above S, a line of layer S itself that must come behind it)
SKIPS = {
    "a": [(0, SELF_POOL, "then gated by layer 0's output", 2, "wgrad conv3x3 8x8x3->32")],
    "b": [(1, SELF_CONV, "ungated: layer 1 is a pool", 2, "pool-bwd 8x8x32")],
    "c": [(5, SELF_HERE, "then gated by layer 5's output", 2, "bn-bwd-reduce"), (1, SELF_CONV, "then gated by layer 1's output", 4, "bn-bwd-reduce")],
    "d": [(0, SELF_POOL, "then gated by layer 0's output", 2, "wgrad conv3x3 32x32x3->32")],
}


def _tags(lines):
    return [l.split(":")[0].split()[0] for l in lines]


@pytest.mark.parametrize("precision", ["fp32", "bf16"])
@pytest.mark.parametrize("name", sorted(RES_NETS))
def test_training_plan_names_the_skip_launches(convnet, name, precision):
    in_shape, layers, B = RES_NETS[name]
    lines = plan_lines(convnet.plan(in_shape, layers, B, precision))
    tags = _tags(lines)
    sk = skips(layers)
    # forward: one bn-add-relu line per block, directly behind its bn-stats line, naming its source
    adds = [i for i, t in enumerate(tags) if t == "bn-add-relu"]
    assert len(adds) == len(sk) and tags.count("bn-relu") == sum(l[0] == "bn_relu" for l in layers)
    for i, (li, s) in zip(adds, sorted(sk.items())):
        assert tags[i - 1] == "bn-stats" and "k_bn_apply_add_relu," in lines[i] and lines[i].endswith(f"skip: the output of layer {s})"), lines[i]
        H, W = (in_shape[0], in_shape[1]) if name != "b" else (4, 4)
        assert lines[i].startswith(f"bn-add-relu {H}x{W}x32:"), lines[i]
    # backward: one skip-bwd line per block, directly behind the input-gradient launch of layer S + 1 and in front of every line of layer S
    at = [i for i, t in enumerate(tags) if t == "skip-bwd"]
    assert len(at) == len(SKIPS[name]) == len(sk) and min(at) > max(adds)
    for i, (s, self_gate, src_gate, bn_before, later) in zip(at, SKIPS[name]):
        assert "k_skip_bwd_add," in lines[i] and f"into layer {s}'s gradient (the skip's gradient {self_gate}; {src_gate})" in lines[i], lines[i]
        pool_source = layers[s][0] == "pool"
        assert lines[i - 1].startswith("conv3x3") and (" epi 0:" if pool_source else " epi 3:") in lines[i - 1], lines[i - 1]
        assert lines[i + 1].startswith("wgrad conv3x3"), lines[i + 1]          # layer S + 1's weight gradient: the same iteration of the walk
        assert tags[:i].count("bn-bwd-reduce") == bn_before, (tags[:i].count("bn-bwd-reduce"), bn_before)
        assert any(x.startswith(later) for x in lines[i + 2:]) and (later == "bn-bwd-reduce" or not any(x.startswith(later) for x in lines[:i])), later
    # the batch-normalisation half is what it was: reduce then dx per layer, no k_relu_bwd
    assert tags.count("bn-bwd-reduce") == tags.count("bn-bwd-dx") == sum(l[0] in ("bn_relu", "bn_add_relu") for l in layers)
    assert not any("k_relu_bwd" in x for x in lines)
    n_par = sum(l[0] != "pool" for l in layers)
    assert lines[-1].startswith("update: k_reduce_all,") and f" {n_par} layers' slabs in one launch" in lines[-1], lines[-1]


def test_net_d_streams_past_the_grid_cap(convnet):
    """n4 = rows x channels / 4 pieces of 16 bytes is more than 4096 workgroups x 256 threads: the grid is capped and some threads loop"""
    in_shape, layers, B = RES_D
    n4 = B * in_shape[0] * in_shape[1] * 32 // 4
    assert n4 == 1064960 and 4096 * 256 < n4 < 2 * 4096 * 256
    lines = plan_lines(convnet.plan(in_shape, layers, B))
    for tag in ("bn-add-relu", "skip-bwd"):
        line, = [x for x in lines if x.startswith(tag)]
        assert ", 4096 workgroups" in line, line
    assert any(x.startswith("bn-stats") and "416 partials of 320 rows" in x for x in lines)
    assert convnet.bn_partials(B * 32 * 32)[0] == 416


@pytest.mark.parametrize("name", sorted(RES_NETS))
def test_eval_plan_adds_the_skip_and_has_no_backward(convnet, name):
    in_shape, layers, B = RES_NETS[name]
    lines = plan_lines(convnet.plan_eval(in_shape, layers, B))
    adds = [x for x in lines if x.startswith("bn-add-relu")]
    assert len(adds) == len(skips(layers))
    assert all("k_bn_apply_add_relu<eval>" in x and "scale and shift from the running statistics" in x and "skip: the output of layer" in x for x in adds), adds
    assert not any("skip-bwd" in x or "bn-stats" in x for x in lines)


def test_bucket_plan_keeps_the_add_in_the_iteration_of_the_layer_above_the_source(convnet):
    in_shape, layers, B = RES_C
    lines = [l.strip() for l in convnet.plan(in_shape, layers, B, buckets=0).splitlines()]
    for s in (5, 1):
        i, = [k for k, x in enumerate(lines) if x.startswith("skip-bwd") and f"into layer {s}'s gradient" in x]
        opened = [x for x in lines[:i] if x.startswith("bucket") and "done" not in x][-1]
        assert opened == f"bucket {10 - (s + 1)}: layers {s + 1} .. {s + 1}", opened       # every layer of net c has parameters: bucket k is layer 10 - k


REFUSALS = [
    # (layers on a 4 x 4 x 32 input, status, layer index named, a word of the message)
    ((("conv", 32), ("conv", 32), ("bn_add_relu", 2), ("dense", 4)), -2, 2, "directly follow"),
    ((("conv", 32), ("conv_linear", 32), ("bn_add_relu", 1), ("dense", 4)), -1, 2, "at least 2"),
    ((("conv", 32), ("conv_linear", 32), ("bn_add_relu", 0), ("dense", 4)), -1, 2, "at least 2"),
    ((("conv", 32), ("conv_linear", 32), ("bn_add_relu", 3), ("dense", 4)), -2, 2, "net's input"),
    ((("conv_linear", 32), ("bn_relu",), ("conv_linear", 32), ("bn_relu",), ("conv_linear", 32), ("bn_add_relu", 3), ("dense", 4)), -2, 5, "not yet normalised"),
    ((("conv", 32), ("conv_linear", 64), ("bn_add_relu", 2), ("dense", 4)), -2, 2, "output shape"),
    ((("conv", 32), ("conv", 32), ("pool",), ("conv_linear", 32), ("bn_add_relu", 4), ("dense", 4)), -2, 4, "output shape"),
    ((("conv", 32), ("pool",), ("conv_linear", 32), ("bn_add_relu", 3), ("dense", 4)), -2, 3, "max-pool behind it"),
    ((("conv", 32), ("conv_linear", 32), ("bn_add_relu", 2), ("conv_linear", 32), ("bn_add_relu", 4), ("dense", 4)), -3, 4, "one skip per source"),
]


@pytest.mark.parametrize("layers,status,index,word", REFUSALS, ids=[f"{r[1]}-{r[3].replace(' ', '-')}-{k}" for k, r in enumerate(REFUSALS)])
def test_refusals_name_the_layer_and_the_reason(convnet, layers, status, index, word):
    for fn in (convnet.plan, convnet.plan_eval):
        with pytest.raises(convnet.ConvNetError, match=rf": {status}: layer {index} \(RCN_HIPX_BN_ADD_RELU\): .*{word}"):
            fn((4, 4, 32), layers, 2)
    with pytest.raises(convnet.ConvNetError, match=rf"rcn_hipx_state_layout: {status}$"):
        convnet.state_layout((4, 4, 32), layers)


def test_bf16_stored_is_refused_with_the_bn_reason(convnet):
    in_shape, layers, B = RES_A
    for fn in (convnet.plan, convnet.plan_eval):
        with pytest.raises(convnet.ConvNetError, match=r"-3: .*batch normalisation"):
            fn(in_shape, layers, B, "bf16_stored")


def test_conv_linear_must_still_be_followed_by_a_bn_kind(convnet):
    with pytest.raises(convnet.ConvNetError, match=r"-2: .*RCN_HIPX_BN_RELU or RCN_HIPX_BN_ADD_RELU"):
        convnet.plan((4, 4, 32), (("conv", 32), ("conv_linear", 32), ("dense", 4)), 2)


def test_state_layout_carries_the_distance(convnet):
    in_shape, layers, _ = RES_C
    d = convnet.state_layout(in_shape, layers)
    assert convnet.KIND["bn_add_relu"] == 6
    assert [d.layers[i].kind for i in range(d.n_layers)] == [convnet.KIND[l[0]] for l in layers]
    assert (d.layers[5].kind, d.layers[5].out) == (6, 4) and (d.layers[9].kind, d.layers[9].out) == (6, 4) and d.layers[1].out == 32
    assert d.shape_and_layers() == (in_shape, [tuple(l) for l in layers])
    # parameters, offsets and body are those of the same description with bn_relu in place of bn_add_relu
    p = convnet.state_layout(in_shape, plain(layers))
    assert d.n_log == p.n_log == n_logical(in_shape, layers) and list(d.layer_off) == list(p.layer_off) and d.body_bytes == p.body_bytes
    assert d.layer_off[5] == tensor_slices(in_shape, layers)[5][0].start
    # a file round-trips the description
    body = np.zeros(int(d.body_bytes), dtype=np.uint8)
    d2, body2, extra = convnet.read_state_file(convnet.write_state_file(d, body, b"x"))
    assert d2.shape_and_layers() == (in_shape, [tuple(l) for l in layers]) and extra == b"x" and body2.size == body.size


def test_hbm_floor_counts_the_skip(convnet):
    """the skip's extra read in the forward (one map) and the add pass (two maps read, one written): four maps of B x 8 x 8 x 32 floats"""
    floor = convnet.ConvNet.step_hbm_floor_bytes
    mk = lambda layers: type("N", (), {"in_shape": RES_A[0], "layers": [tuple(l) for l in layers]})()
    assert floor(mk(RES_A[1]), 5) - floor(mk(plain(RES_A[1])), 5) == 5 * 4 * (8 * 8 * 32 * 4)


def test_res_ref_on_a_hand_computed_case():
    """A 1 x 1 map of 32 channels, two rows, every convolution its centre tap = identity (bias 0), so the channels stay apart:
    conv (ReLU) -> block -> dense 1, weighted sum of the two logits L = 1 z_0 + 2 z_1.  Per channel, with s = (s_0, s_1) > 0 the source's
    output and eps = 0.25: batch normalisation of two values (u_0, u_1) has r = (u_0 - u_1) / 2, xh = (h, -h), h = r / sqrt(r^2 + eps), and
    its backward is dx_0 = -dx_1 = gamma eps (dy_0 - dy_1) / 2 / (r^2 + eps)^1.5.
        y2 = b1 +- g1 h1 (b1 = 2 keeps both open)        y4 = relu(b2 +- g2 h2 + s),  h2 from r2 = g1 h1
    Channel 0 has b2 = -s_1 - 1 and s_0 = s_1 + 3: its row 1 is shut (y4 = 0), its row 0 open.
    dL/dy4[n] = v_n w (v = (1, 2), w the dense weight), dsum = dL/dy4 where y4 > 0; the source's gradient is the SUM of the skip's share,
    dsum, and the main path's, bn1_backward(bn2_backward(dsum))."""
    C, eps = 32, 0.25
    rng = np.random.default_rng(0)
    s = np.stack([1.0 + rng.random(C), 1.0 + rng.random(C)])                 # (row, channel), positive
    s[0, 0] = s[1, 0] + 3.0
    g1, b1 = 0.5 + rng.random(C), np.full(C, 2.0)
    g2, b2 = 0.5 + rng.random(C), 1.0 + 0.1 * rng.standard_normal(C)
    b2[0] = -s[1, 0] - 1.0
    w, v = rng.standard_normal(C), np.array([1.0, 2.0])
    eye = np.zeros((9 * C, C)); eye[4 * C:5 * C] = np.eye(C)
    layers = (("conv", C),) + block(C) + (("dense", 1),)
    flat = np.concatenate([eye.ravel(), np.zeros(C), eye.ravel(), np.zeros(C), g1, b1, eye.ravel(), np.zeros(C), g2, b2, w, [0.5]])
    net = TorchNet((1, 1, C), layers, flat, eps=eps)
    z = net.forward(s.reshape(2, 1, 1, C), True)
    net.outs[0].retain_grad()
    (z[:, 0] * net.torch.from_numpy(v)).sum().backward()
    # by hand
    r1 = (s[0] - s[1]) / 2
    h1 = r1 / np.sqrt(r1 ** 2 + eps)
    y2 = np.stack([b1 + g1 * h1, b1 - g1 * h1])
    assert (y2 > 0).all()
    r2 = g1 * h1
    h2 = r2 / np.sqrt(r2 ** 2 + eps)
    y4 = np.maximum(0.0, np.stack([b2 + g2 * h2, b2 - g2 * h2]) + s)
    assert y4[1, 0] == 0.0 and y4[0, 0] > 0.0 and (y4[:, 1:] > 0).all()
    assert np.allclose(net.outs[4].detach().numpy().reshape(2, C), y4, rtol=0, atol=1e-12)
    assert np.allclose(z.detach().numpy().ravel(), y4 @ w + 0.5, rtol=0, atol=1e-12)
    dsum = (y4 > 0) * v[:, None] * w[None, :]
    dy2_0 = g2 * eps * (dsum[0] - dsum[1]) / 2 / (r2 ** 2 + eps) ** 1.5
    main_0 = g1 * eps * (dy2_0 - -dy2_0) / 2 / (r1 ** 2 + eps) ** 1.5
    want = dsum + np.stack([main_0, -main_0])
    got = net.outs[0].grad.numpy().reshape(2, C)
    assert np.allclose(got, want, rtol=0, atol=1e-12), np.abs(got - want).max()
    assert np.abs(main_0).min() > 1e-4 and np.abs(dsum).max() > 0.1          # both paths carry something: neither could be dropped unnoticed
    # without the source's gate on the skip path the VALUES are the same (gate_source only changes the gradient)
    loose = TorchNet((1, 1, C), layers, flat, eps=eps, gate_source=False)
    assert np.array_equal(loose.forward(s.reshape(2, 1, 1, C), True).detach().numpy(), z.detach().numpy())
    assert np.array_equal(net.params(), flat)
