"""GPU tests of the fp32 LDS-tiled Track-X kernels (csrc/convnet_halo.hpp) against the f64 oracle, with the tiling mode forced to
"lds" so that the small shapes an oracle can afford reach them (in "auto" mode small layers take the split-K implicit GEMM).
Shapes are chosen for the kernels' corner cases: both block geometries (8 x 16 of one image, 8 x 8 of two images with an odd
batch), maps that do not fill their blocks, one / two input-channel blocks, 32- and 64-wide column blocks, the fused pool epilogue,
pooled-resolution gradients into the input-gradient and weight-gradient kernels, the first layer with 1 and 3 channels.
No reference counterpart ("parity unpinned"); tolerance as tests/test_gpu_convnet.py: |d| <= 2e-4 * scale + 1e-6."""
import numpy as np
import pytest
from _convnet_util import FUSED_HEAD, HALO_NETS, close, close_per_tensor, make_net, oracle_params

from oracle import convnet_oracle as co

pytestmark = pytest.mark.gpu

NETS = HALO_NETS                                        # (tests/_convnet_util.py: the table, with what each net is there for)


def _setup(in_shape, layers, B, tiling):
    import torch
    rng = np.random.default_rng(B + in_shape[0])
    net = make_net((in_shape, layers, B), precision=None, tiling=tiling)
    _, _, flat, w32, b32 = oracle_params(rng, in_shape, layers)
    net.set_params(flat)
    x = rng.standard_normal((B,) + in_shape).astype(np.float32)
    y = rng.integers(0, layers[-1][1], B).astype(np.int32)
    return torch, net, flat, x, y, w32, b32


@pytest.mark.parametrize("in_shape,layers,B", NETS)
def test_lds_tiled_kernels_match_oracle(in_shape, layers, B):
    torch, net, flat, x, y, w32, b32 = _setup(in_shape, layers, B, "lds")
    xd, yd = net.to_device(x), net.to_device(y)
    x64 = x.astype(np.float64)
    loss_ref, logits_ref, gws, gbs = co.loss_and_grads(x64, y, w32, b32, layers)
    with torch.cuda.stream(net.stream):
        logits = net.forward(xd)
        loss = torch.zeros(1, dtype=torch.float32, device=net.device)
        grad = net.gradients(xd, yd, loss=loss)
    net.synchronize()
    close(logits.cpu().numpy(), logits_ref)
    assert abs(loss.item() - loss_ref) <= 2e-4 * max(1.0, loss_ref)
    g1 = net.unpad(grad)
    close_per_tensor(g1, co.flatten(gws, gbs), in_shape, layers)      # every layer's weights and biases at their own scale
    # fixed summation orders: a second evaluation is bit-identical
    with torch.cuda.stream(net.stream):
        grad2 = net.gradients(xd, yd)
    net.synchronize()
    assert np.array_equal(net.unpad(grad2), g1)
    # one SGD step eagerly, the second as a replayed graph
    lr = 0.05
    with torch.cuda.stream(net.stream):
        net.train_step(xd, yd, lr, loss)
    net.synchronize()
    nw, nb, _ = co.sgd_step(x64, y, w32, b32, layers, lr)
    close_per_tensor(net.get_params(), co.flatten(nw, nb), in_shape, layers)
    with torch.cuda.stream(net.stream):
        net.train_step(xd, yd, lr, loss)
    net.synchronize()
    nw2, nb2, l2 = co.sgd_step(x64, y, nw, nb, layers, lr)
    close(net.get_params(), co.flatten(nw2, nb2), rtol=4e-4)
    assert abs(loss.item() - l2) <= 4e-4 * max(1.0, l2)


@pytest.mark.parametrize("in_shape,layers,B", NETS[:3])
def test_tiling_modes_agree(in_shape, layers, B):
    """The three modes are three routes to the same numbers: the implicit-GEMM kernels and the LDS-tiled ones differ only in the
    order of the fp32 sums (and agree on every pooling arg-max here: the logits would show a flipped window).  The third net ends in
    ReLU-dense -> logits: outside "gemm" mode its classifier head is ONE launch (k_head_f32), in "gemm" mode five."""
    out = {}
    for mode in ("gemm", "auto", "lds"):
        torch, net, flat, x, y, _, _ = _setup(in_shape, layers, B, mode)
        xd, yd = net.to_device(x), net.to_device(y)
        with torch.cuda.stream(net.stream):
            logits = net.forward(xd)
            grad = net.gradients(xd, yd)
        net.synchronize()
        out[mode] = (logits.cpu().numpy(), net.unpad(grad))
        net.close()
    for mode in ("auto", "lds"):
        close(out[mode][0], out["gemm"][0], rtol=1e-5)
        close(out[mode][1], out["gemm"][1], rtol=2e-5)


def test_fused_head_loss_of_257_workgroups_agrees_with_the_plain_path():
    """B = 8193 on FUSED_HEAD: 257 workgroups of 32 samples, the last with one, so "thread 0" of the last-arriving workgroup takes the
    partials of blocks 0 and 256.  The head sums a row's exponentials with 8 lanes, the plain path (option head = 0: k_softmax_ce) with 32,
    so the two losses are held as test_tiling_modes_agree holds two routes to the same logits: rtol 1e-5."""
    in_shape, layers, _ = FUSED_HEAD
    B = 8193
    loss = {}
    for head in (1, 0):
        torch, net, flat, x, y, _, _ = _setup(in_shape, layers, B, "auto")
        net.set_option("head", head)
        plan = net.plan_of_this_net(B)
        assert ("k_head_f32, 257 workgroups" if head else "k_softmax_ce, 1025 workgroups") in plan, plan
        xd, yd = net.to_device(x), net.to_device(y)
        with torch.cuda.stream(net.stream):
            out = torch.zeros(1, dtype=torch.float32, device=net.device)
            net.gradients(xd, yd, loss=out)
        net.synchronize()
        loss[head] = out.item()
        net.close()
    print("fused", repr(loss[1]), "plain", repr(loss[0]))
    close([loss[1]], [loss[0]], rtol=1e-5)


def test_set_tiling_rejects_unknown_modes():
    from mercer_research_amd.convnet import ConvNet, ConvNetError
    net = ConvNet((8, 8, 3), (("conv", 32), ("pool",), ("dense", 10)), 2)
    with pytest.raises(ConvNetError):
        net._ck(net.lib.rcn_hipx_set_tiling(net.net, 7))


@pytest.mark.parametrize("in_shape,layers,B", [NETS[0], NETS[2]])
def test_backward_overlap_changes_nothing_but_the_schedule(in_shape, layers, B):
    """The weight gradients of the backward pass run on a second stream beside the input-gradient chain (rcn_hipx_set_overlap):
    same kernels, same summation orders -- parameters after three steps (one eager, two replayed graphs) are bit-identical."""
    out = []
    for on in (True, False):
        torch, net, flat, x, y, _, _ = _setup(in_shape, layers, B, "lds")
        net.set_overlap(on)
        xd, yd = net.to_device(x), net.to_device(y)
        loss = torch.zeros(1, dtype=torch.float32, device=net.device)
        with torch.cuda.stream(net.stream):
            for _ in range(3):
                net.train_step(xd, yd, 0.05, loss)
        net.synchronize()
        out.append((net.get_params(), loss.item()))
        net.close()
    assert np.array_equal(out[0][0], out[1][0])
    assert out[0][1] == out[1][1]
