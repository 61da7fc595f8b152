"""What the GPU files that hold a net to its float64 torch twin share (tests/test_gpu_convnet_res.py, tests/test_gpu_convnet_gap.py,
tests/test_gpu_convnet_deep.py) and the CPU files that prepare the twin's side (tests/test_convnet_gap_plan.py,
tests/test_convnet_deep_plan.py): one schedule -- a gradients call, `steps` plain SGD steps, a forward and an evaluation on the running
statistics -- run on the device (`device_run`) and on a twin (`twin_schedule`), their comparison quantity by quantity (`compare`), and ONE
update of an optimiser family against torch.optim on the twin (`against_torch`).  Not a test file and not a conftest: every assert
carries its message."""
import numpy as np
from _convnet_util import LR, close, dev, make_net, same_bits, step
from _torch_ref import TorchNet, close_per_tensor, random_params


def grads(net, xd, yd, B):
    """(logical gradient, loss, training logits) of one gradients call"""
    import torch
    loss = torch.zeros(1, dtype=torch.float32, device=net.device)
    with torch.cuda.stream(net.stream):
        g = net.gradients(xd, yd, loss=loss)
        z = net.last_logits(B)
    net.synchronize()
    return net.unpad(g), float(loss.item()), z.cpu().numpy()


def stats(net):
    return net.get_bn_stats() if net.get_bn()[2] else np.zeros(0, dtype=np.float32)


def device_run(spec, precision, flat, x, y, steps, tiling=None, options=()):
    """What the device makes of twin_schedule's schedule"""
    import torch
    B = spec[2]
    net = make_net(spec, precision, tiling=tiling)
    for k, v in options:
        net.set_option(k, v)
    net.set_params(flat)
    xd, yd = dev(net, x), dev(net, y)
    out = {}
    out["grad"], out["loss"], out["logits"] = grads(net, xd, yd, B)
    out["stats1"] = stats(net)
    loss = torch.zeros(1, dtype=torch.float32, device=net.device)
    out["losses"] = []
    for _ in range(steps):
        step(net, xd, yd, LR, loss)
        out["losses"].append(float(loss.item()))
    out["params"], out["stats"] = net.get_params(), stats(net)
    with torch.cuda.stream(net.stream):
        ze = net.forward(xd)
    net.synchronize()
    out["eval_logits"] = ze.cpu().numpy()
    out["eval"] = net.evaluate(xd, yd, x_scale=1.0, x_shift=0.0)
    net.close()
    return out


def twin_schedule(ref, x, y, steps):
    """What a twin (tests/_torch_ref.py) makes of the schedule: one gradients call, `steps` plain SGD steps at LR, then a
    forward and an evaluation on the running statistics; and the margin between a row's two best evaluation logits with their scale"""
    B = len(y)
    out = {}
    out["loss"], out["logits"], out["grad"] = ref.loss_and_grads(x, y)
    out["stats1"] = ref.bn_stats().copy()
    out["losses"] = [ref.sgd_step(x, y, LR) for _ in range(steps)]
    out["params"], out["stats"] = ref.params(), ref.bn_stats().copy()
    zr = out["eval_logits"] = ref.logits(x, train=False)
    lse = np.log(np.exp(zr - zr.max(1, keepdims=True)).sum(1)) + zr.max(1)
    out["eval"] = (float((lse - zr[np.arange(B), y]).mean()), int((zr.argmax(1) == y).sum()))
    top = np.sort(zr, axis=1)
    out["margin"], out["scale"] = float(np.min(top[:, -1] - top[:, -2])), float(np.abs(zr).max())
    return out


def compare(spec, r, ref, rtol, rtol2, steps, tag, unrounded_logits=None, widened_gradients=None):
    """Every quantity of a device_run `r` against the twin_schedule `ref` of the same data: rtol of a tensor's scale + 1e-6 for what one
    pass makes, rtol2 for what a second step has touched.  unrounded_logits: (the unrounded twin's training logits, their bound) for a bf16
    run.  widened_gradients: _torch_ref.close_per_tensor's `widened`, for the gradient alone.  The correct count is always compared: the
    caller's CPU file asserts the margin from the twin alone.  Prints and returns the worst share of an allowance."""
    t = tag
    used = [close(r["logits"], ref["logits"], rtol, f"{t} training logits"), close([r["loss"]], [ref["loss"]], rtol, f"{t} loss")]
    if unrounded_logits is not None:
        close(r["logits"], unrounded_logits[0], unrounded_logits[1], f"{t} training logits against the unrounded twin")
    assert np.isfinite(r["grad"]).all(), f"{t}: a gradient is not finite"
    used.append(close_per_tensor(r["grad"], ref["grad"], spec[0], spec[1], rtol, f"{t} gradient", widened=widened_gradients))
    if ref["stats"].size:
        used.append(close(r["stats1"], ref["stats1"], rtol, f"{t} running statistics after gradients()"))
        used.append(close(r["stats"], ref["stats"], rtol2, f"{t} running statistics after {steps} steps"))
    assert len(r["losses"]) == steps == 2, (t, len(r["losses"]), steps)
    used.append(close([r["losses"][0]], [ref["losses"][0]], rtol, f"{t} loss of step 1"))
    used.append(close([r["losses"][1]], [ref["losses"][1]], rtol2, f"{t} loss of step 2"))
    used.append(close_per_tensor(r["params"], ref["params"], spec[0], spec[1], rtol2, f"{t} parameters after {steps} steps"))
    used.append(close(r["eval_logits"], ref["eval_logits"], rtol2, f"{t} evaluation logits"))
    (loss, correct), (rloss, rcorrect) = r["eval"], ref["eval"]
    used.append(close([loss], [rloss], rtol2, f"{t} evaluation loss"))
    assert ref["margin"] > 4 * rtol2 * ref["scale"], (t, ref["margin"], ref["scale"])
    assert correct == rcorrect, (t, correct, rcorrect)
    print(f"{t}: worst share of an allowance = {max(used):.3f}")
    return max(used)


def update_case(spec, micro=1):
    """(parameters, `micro` batches) of against_torch's one update: seeds 6 and 11"""
    in_shape, layers, B = spec
    flat = random_params(np.random.default_rng(6), in_shape, layers)
    rng = np.random.default_rng(11)
    return flat, [(rng.standard_normal((B,) + in_shape).astype(np.float32), rng.integers(0, layers[-1][1], B).astype(np.int32)) for _ in range(micro)]


def twin_update(ref, data, make_optim):
    """ONE update of the twin `ref` over the micro-batches of `data` by make_optim(parameters) = (the torch optimiser, the step rate, the
    clipping norm or None); returns the step rate"""
    import torch
    opt, lr, clip = make_optim(ref.parameters())
    opt.zero_grad()
    for x, y in data:
        z = ref.forward(x, True)
        (torch.nn.functional.cross_entropy(z, torch.from_numpy(y.astype(np.int64))) / len(data)).backward()
    if clip:
        torch.nn.utils.clip_grad_norm_(ref.parameters(), clip)
    opt.step()
    return lr


def against_torch(spec, configure, make_optim, micro=1, rtol=4e-4, tag="", widened=None):
    """ONE update of `micro` micro-batches on the net `spec` on the device and in float64 torch (the twin):
    parameters per tensor and running statistics at the bound of tests/test_gpu_convnet_bn_recipe.py.  widened: _torch_ref.close_per_tensor's,
    for the parameters."""
    in_shape, layers, B = spec
    flat, data = update_case(spec, micro)
    net = make_net(spec, "fp32")
    net.set_params(flat)
    configure(net)
    ref = TorchNet(in_shape, layers, flat)
    lr = twin_update(ref, data, make_optim)
    for x, y in data:
        step(net, dev(net, x), dev(net, y), lr)
    assert not same_bits(net.get_params(), flat), f"{tag}: the update changed nothing"
    worst = close_per_tensor(net.get_params(), ref.params(), in_shape, layers, rtol, f"{tag} parameters", widened=widened)
    worst = max(worst, close(net.get_bn_stats(), ref.bn_stats(), rtol, f"{tag} running statistics"))
    print(f"{tag}: worst share of an allowance = {worst:.3f}")
    net.close()
