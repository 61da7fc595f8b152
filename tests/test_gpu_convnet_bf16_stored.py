"""GPU tests of Track X's bf16-storage mode (rcn_hipx_set_precision "bf16_stored": the convolutional stage's activations and gradients
live in HBM as bf16): against bf16 mode bit for bit where the rounding only moves, against the oracle with the storage rounding mirrored,
the 16 x 16 pixel-block form, partial batches and mode switches, and the nets the mode refuses."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu


def _layer_slices(in_shape, layers):
    """(kind, w slice, b slice) of every layer with parameters in the logical flat layout (W[K][Cout] then b[Cout], layers back to back)."""
    H, W, Cc = in_shape
    off, out, flat = 0, [], False
    for l in layers:
        if l[0] == "conv":
            k, o = 9 * Cc, l[1]
            Cc = o
        elif l[0] == "pool":
            H, W = H // 2, W // 2
            continue
        else:
            k, o = (Cc if flat else H * W * Cc), l[1]
            Cc, flat = o, True
        out.append((l[0], slice(off, off + k * o), slice(off + k * o, off + k * o + o)))
        off += k * o + o
    return out


@pytest.mark.parametrize("shape", ["pool_pairs", "conv_conv"])
def test_trackx_bf16_storage_rounds_what_bf16_mode_rounds(shape):
    """RCN_HIPX_BF16_STORED: the convolutional stage's activations and gradients live in HBM as bf16.  Every consumer
    of those tensors rounds them to bf16 on the way into LDS in bf16 mode anyway, so storing them rounded changes WHERE the rounding
    happens, not what is rounded: logits and loss equal bf16 mode's bit for bit, and so does the weight gradient of every layer but the
    first (whose fp32 kernel now reads a rounded dZ); bias gradients (summed in fp32 from dZ) and the first layer's weights agree to bf16
    resolution.  Then ten training steps in each mode end at the same loss to 2 %."""
    import torch
    from mercer_research_amd.convnet import ConvNet
    if shape == "pool_pairs":
        in_shape, layers, B = (16, 16, 3), (("conv", 32), ("pool",), ("conv", 64), ("pool",), ("dense_relu", 128), ("dense", 10)), 64
    else:
        in_shape, layers, B = (32, 32, 1), (("conv", 32), ("conv", 32), ("pool",), ("conv", 64), ("conv", 128), ("pool",), ("dense", 10)), 128    # (a batch at which bf16 mode does not split K either: same sums)
    rng = np.random.default_rng(17)
    x = rng.standard_normal((B,) + in_shape).astype(np.float32)
    y = rng.integers(0, 10, B).astype(np.int32)
    res = {}
    for mode in ("bf16", "bf16_stored"):
        net = ConvNet(in_shape, layers, B)
        net.init_params(9)
        net.set_precision(mode)
        plan = net.plan_of_this_net(B)
        assert ("stored as bf16" in plan) == (mode == "bf16_stored"), plan
        xd, yd = net.to_device(x), net.to_device(y)
        logits_d = net.forward(xd)
        net.synchronize()
        logits = logits_d.cpu().numpy().copy()
        loss = torch.zeros(1, dtype=torch.float32, device=net.device)
        g = net.gradients(xd, yd, None, loss)
        net.synchronize()
        grad, l0 = net.unpad(g), float(loss.item())
        for _ in range(10):
            net.train_step(xd, yd, 0.02, loss)
        net.synchronize()
        res[mode] = (logits, l0, grad, float(loss.item()))
        net.close()
    a, b = res["bf16"], res["bf16_stored"]
    assert np.array_equal(a[0], b[0]) and a[1] == b[1], (a[1], b[1])
    assert np.isfinite(b[2]).all() and np.abs(b[2]).max() > 0
    for li, (kind, ws, bs) in enumerate(_layer_slices(in_shape, layers)):
        if li > 0:
            assert np.array_equal(a[2][ws], b[2][ws]), (li, kind, float(np.abs(a[2][ws] - b[2][ws]).max()))
        else:
            assert np.linalg.norm(a[2][ws] - b[2][ws]) <= 1e-2 * np.linalg.norm(a[2][ws]), (li, kind)
        assert np.linalg.norm(a[2][bs] - b[2][bs]) <= 1e-2 * np.linalg.norm(a[2][bs]) + 1e-7, (li, kind)
    assert b[3] < b[1] and abs(a[3] - b[3]) <= 2e-2 * abs(a[3]), (a[1], a[3], b[3])


@pytest.mark.parametrize("in_shape,layers,B", [
    ((16, 16, 3), (("conv", 32), ("pool",), ("conv", 64), ("pool",), ("dense_relu", 32), ("dense", 10)), 5),
    ((32, 32, 1), (("conv", 32), ("conv", 32), ("pool",), ("conv", 64), ("pool",), ("dense", 7)), 3),
    ((16, 32, 3), (("conv", 64), ("pool",), ("conv", 128), ("conv", 128), ("pool",), ("dense_relu", 128), ("dense_relu", 32), ("dense", 3)), 9),
    # 24-pixel-wide maps: the first layer's kernels take 8 x 8 blocks of TWO images side by side (an odd batch leaves the last block half empty)
    ((24, 24, 3), (("conv", 32), ("pool",), ("conv", 64), ("pool",), ("dense_relu", 64), ("dense", 10)), 5),
    ((24, 24, 1), (("conv", 32), ("conv", 32), ("pool",), ("dense", 10)), 6),
])
def test_trackx_bf16_storage_matches_the_oracle_with_the_storage_rounding_mirrored(in_shape, layers, B):
    """RCN_HIPX_BF16_STORED against oracle/convnet_oracle.py evaluated with the same operand rounding AND the same storage rounding
    (stored=True: maps rounded where they are written, gradients with respect to maps rounded where the input-gradient kernel writes
    them): logits, loss, every gradient and two training steps within the tolerances of the bf16-operand test (5e-3 of each tensor's
    scale; 2e-2 after two steps)."""
    import torch
    from mercer_research_amd.convnet import ConvNet
    from oracle import convnet_oracle as co
    rng = np.random.default_rng(B + 3)
    net = ConvNet(in_shape, layers, B)
    shapes = co.param_shapes(in_shape, layers)
    ws = [rng.standard_normal(k) * np.sqrt(2.0 / k[0]) for k, _ in shapes]
    bs = [rng.standard_normal(n) * 0.1 for _, n in shapes]
    net.set_params(co.flatten(ws, bs).astype(np.float32))
    x = rng.standard_normal((B,) + in_shape)
    y = rng.integers(0, layers[-1][1], B).astype(np.int32)
    xd, yd = net.to_device(x.astype(np.float32)), net.to_device(y)
    x64 = x.astype(np.float32).astype(np.float64)
    w32 = [w.astype(np.float32).astype(np.float64) for w in ws]
    b32 = [b.astype(np.float32).astype(np.float64) for b in bs]
    loss_ref, logits_ref, gws, gbs = co.loss_and_grads(x64, y, w32, b32, layers, operand="bf16", stored=True)
    net.set_precision("bf16_stored")

    def close(a, b, rtol):
        scale = max(1e-3, float(np.abs(b).max()))                      # (tests/test_gpu_convnet.py _close: of each tensor's scale)
        assert np.abs(np.asarray(a, dtype=np.float64) - b).max() <= rtol * scale + 1e-6, (float(np.abs(np.asarray(a, dtype=np.float64) - b).max()), scale)
    logits = net.forward(xd)
    loss = torch.zeros(1, dtype=torch.float32, device=net.device)
    grad = net.gradients(xd, yd, loss=loss)
    net.synchronize()
    close(logits.cpu().numpy(), logits_ref, 5e-3)
    assert abs(loss.item() - loss_ref) <= 5e-3 * max(1.0, loss_ref)
    got, ref = net.unpad(grad), co.flatten(gws, gbs)
    for kind, wsl, bsl in _layer_slices(in_shape, layers):
        close(got[wsl], ref[wsl], 5e-3)
        close(got[bsl], ref[bsl], 5e-3)
    net.train_step(xd, yd, 0.05, loss)
    net.train_step(xd, yd, 0.05, loss)
    net.synchronize()
    nw, nb, _ = co.sgd_step(x64, y, w32, b32, layers, 0.05, operand="bf16", stored=True)
    nw, nb, _ = co.sgd_step(x64, y, nw, nb, layers, 0.05, operand="bf16", stored=True)
    close(net.get_params(), co.flatten(nw, nb), 2e-2)
    net.close()


def test_trackx_bf16_storage_16x16_pixel_blocks_compute_the_same_bits():
    """Option "bf16_rows16": k_conv3x3_halo_bf16p<..., MG = 2> -- a wave computes two 32-pixel row groups against the same staged weights.
    Same operands, same accumulation order per output: logits, loss, gradients and three training steps equal the 8-row form's bit for
    bit, and the plan names the form for the layers whose height it covers without extra padding."""
    import torch
    from mercer_research_amd.convnet import ConvNet
    in_shape, layers, B = (32, 32, 3), (("conv", 32), ("conv", 64), ("pool",), ("conv", 64), ("conv", 128), ("pool",), ("dense_relu", 64), ("dense", 10)), 128
    rng = np.random.default_rng(23)
    x = rng.standard_normal((B,) + in_shape).astype(np.float32)
    y = rng.integers(0, 10, B).astype(np.int32)
    res = []
    for rows16 in (0, 1):
        net = ConvNet(in_shape, layers, B)
        net.init_params(4)
        net.set_option("bf16_rows16", rows16)
        net.set_precision("bf16_stored")
        plan = net.plan_of_this_net(B)
        assert ("16 x 16 pixel blocks" in plan) == bool(rows16), plan
        xd, yd = net.to_device(x), net.to_device(y)
        logits = net.forward(xd)
        loss = torch.zeros(1, dtype=torch.float32, device=net.device)
        g = net.gradients(xd, yd, None, loss)
        net.synchronize()
        out = [logits.cpu().numpy().copy(), float(loss.item()), g.cpu().numpy().copy()]
        for _ in range(3):
            net.train_step(xd, yd, 0.002, loss)
        net.synchronize()
        out += [net.get_params(), float(loss.item())]
        res.append(out)
        net.close()
    a, b = res
    assert np.array_equal(a[0], b[0]) and a[1] == b[1] and np.array_equal(a[2], b[2]) and np.array_equal(a[3], b[3]) and a[4] == b[4]
    assert np.isfinite(b[3]).all() and np.isfinite(b[4])
    # the 16-row form on a grid smaller than its item count ("halo_f32_slots"): every workgroup walks several items, with carries
    for slots in (3, 7):
        net = ConvNet(in_shape, layers, B)
        net.init_params(4)
        net.set_option("bf16_rows16", 1)
        net.set_precision("bf16_stored")
        unforced = net.plan_of_this_net(B)
        net.set_option("halo_f32_slots", slots)
        plan = net.plan_of_this_net(B)
        assert plan == unforced and "16 x 16 pixel blocks" in plan, plan
        xd, yd = net.to_device(x), net.to_device(y)
        logits = net.forward(xd)
        loss = torch.zeros(1, dtype=torch.float32, device=net.device)
        g = net.gradients(xd, yd, None, loss)
        net.synchronize()
        assert np.array_equal(logits.cpu().numpy(), b[0]) and float(loss.item()) == b[1] and np.array_equal(g.cpu().numpy(), b[2]), slots
        net.close()


def test_trackx_bf16_storage_partial_batches_and_mode_switches():
    """A net built for 32 pictures steps batches of 7 and 32 in bf16-storage mode (in this mode a 3 x 3 layer's kernels do not depend on
    the batch size), then is switched to bf16 and fp32 mode and back: every forward pass agrees with the oracle evaluated in that mode on
    the parameters the net has at that point."""
    import torch
    from mercer_research_amd.convnet import ConvNet
    from oracle import convnet_oracle as co
    in_shape, layers, MB = (16, 16, 3), (("conv", 32), ("conv", 32), ("pool",), ("conv", 64), ("pool",), ("dense_relu", 64), ("dense", 10)), 32
    rng = np.random.default_rng(31)
    net = ConvNet(in_shape, layers, MB)
    net.init_params(3)
    net.set_precision("bf16_stored")
    loss = torch.zeros(1, dtype=torch.float32, device=net.device)
    for B in (7, 32, 7):
        x = rng.standard_normal((B,) + in_shape).astype(np.float32)
        y = rng.integers(0, 10, B).astype(np.int32)
        net.train_step(net.to_device(x), net.to_device(y), 0.01, loss)
    net.synchronize()
    assert np.isfinite(loss.item())
    x = rng.standard_normal((7,) + in_shape).astype(np.float32)
    xd = net.to_device(x)
    ws, bs = co.unflatten(net.get_params().astype(np.float64), in_shape, layers)
    for mode, kw, tol in (("bf16_stored", dict(operand="bf16", stored=True), 5e-3), ("bf16", dict(operand="bf16"), 5e-3), ("fp32", dict(), 2e-4),
                          ("bf16_stored", dict(operand="bf16", stored=True), 5e-3)):
        net.set_precision(mode)
        lg = net.forward(xd)
        net.synchronize()
        ref = co.forward(x.astype(np.float64), ws, bs, layers, **kw)
        assert np.abs(lg.cpu().numpy() - ref).max() <= tol * max(1e-3, np.abs(ref).max()) + 1e-6, mode
    net.close()


def test_trackx_bf16_storage_refuses_a_net_it_does_not_cover():
    """rcn_hipx_set_precision walks the net's plan first: a net with a layer that no bf16-tensor kernel runs (here: the LDS-tiled kernels
    switched off) gets -3 with the reason, and stays in the mode it was in."""
    from mercer_research_amd.convnet import ConvNet, ConvNetError
    in_shape, layers, B = (16, 16, 3), (("conv", 32), ("pool",), ("conv", 64), ("pool",), ("dense", 10)), 16
    net = ConvNet(in_shape, layers, B)
    net.init_params(1)
    net.set_precision("bf16")
    net.set_option("halo", 0)
    with pytest.raises(ConvNetError, match="bf16 storage"):
        net.set_precision("bf16_stored")
    assert "stored as bf16" not in net.plan_of_this_net(B)
    net.set_option("halo", 1)
    net.set_precision("bf16_stored")
    assert "stored as bf16" in net.plan_of_this_net(B)
    net.close()
