"""GPU tests of batch normalisation inside the training recipe, on net a of tests/test_convnet_bn_plan.py: determinism of the fixed-order
sums, the epoch's one graph, the running statistics under graph replay, the optimisers, clipping and accumulation against torch in
float64 (tests/_torch_ref.py; the bounds of tests/test_gpu_convnet_bn.py), evaluation on the average, snapshot / restore and save / load."""
import numpy as np
import pytest
from _convnet_util import LR, batches, close, dev, epoch, make_net, same_bits, step, twins
from _torch_ref import TorchNet, close_per_tensor, random_params, tensor_slices
from test_convnet_bn_plan import BN_A

pytestmark = pytest.mark.gpu

IN_SHAPE, LAYERS, B = BN_A
PLAIN_A = (IN_SHAPE, tuple(("conv", l[1]) if l[0] == "conv_linear" else l for l in LAYERS if l[0] != "bn_relu"), B)      # net a without BN


def _host_batches(k, seed=11):
    rng = np.random.default_rng(seed)
    return [(rng.standard_normal((B,) + IN_SHAPE).astype(np.float32), rng.integers(0, LAYERS[-1][1], B).astype(np.int32)) for _ in range(k)]


def _state(net):
    return net.get_params(), net.get_bn_stats(), net.get_velocity()


def _close(*nets):
    for n in nets:
        n.close()


def _same(a, b):
    return all(same_bits(u, v) for u, v in zip(a, b))


def test_twins_are_bit_identical():
    a, b = twins(BN_A, "fp32", 2)
    for x, y in batches(a, BN_A, 3):
        step(a, x, y, LR)
        step(b, x, y, LR)
    assert _same(_state(a), _state(b))
    assert not same_bits(a.get_bn_stats(), np.r_[np.zeros(32), np.ones(32), np.zeros(64), np.ones(64)].astype(np.float32))
    _close(a, b)


def test_epoch_equals_steps_and_adds_no_graph():
    a, b = twins(BN_A, "fp32", 2)
    plain = make_net(PLAIN_A, "fp32")
    plain.init_params(1)
    rng = np.random.default_rng(2)
    n = 4 * B
    X, y = rng.standard_normal((n,) + IN_SHAPE).astype(np.float32), rng.integers(0, 10, n).astype(np.int32)
    perm = rng.permutation(n).astype(np.int32)
    Xd, yd, pd = dev(a, X), dev(a, y), dev(a, perm)
    epoch(a, Xd, yd, pd, B, LR)
    epoch(plain, Xd, yd, pd, B, LR)
    for s in range(4):
        rows = perm[s * B:(s + 1) * B]
        step(b, dev(b, X[rows]), dev(b, y[rows]), LR)
    assert _same(_state(a), _state(b))
    assert a.graphs_instantiated() == plain.graphs_instantiated() == 1
    _close(a, b, plain)


def test_running_statistics_advance_under_graph_replay():
    """The same batch at rate 0 (the parameters stay): the eager step, then k - 1 replays of its graph; after each the running statistics
    are torch's recurrence r <- 0.9 r + 0.1 s."""
    flat = random_params(np.random.default_rng(4), IN_SHAPE, LAYERS)
    (x, y), = _host_batches(1)
    net = make_net(BN_A, "fp32")
    net.set_params(flat)
    ref = TorchNet(IN_SHAPE, LAYERS, flat)
    xd, yd = dev(net, x), dev(net, y)
    seen = [net.get_bn_stats()]
    for k in range(5):
        step(net, xd, yd, 0.0)
        ref.logits(x, train=True)
        seen.append(net.get_bn_stats())
        close(seen[-1], ref.bn_stats(), 2e-4, f"running statistics after {k + 1} forwards")
        assert not np.array_equal(seen[-1], seen[-2])
    assert net.graphs_instantiated() == 1 and same_bits(net.get_params(), flat)
    net.close()


def _against_torch(configure, make_optim, micro=1, updates=2, rtol=4e-4, tag=""):
    """`updates` updates of `micro` micro-batches each on the device and in float64 torch; parameters per tensor and running statistics"""
    import torch
    flat = random_params(np.random.default_rng(6), IN_SHAPE, LAYERS)
    data = _host_batches(micro * updates)
    net = make_net(BN_A, "fp32")
    net.set_params(flat)
    configure(net)
    ref = TorchNet(IN_SHAPE, LAYERS, flat)
    opt, lr, clip = make_optim(ref.parameters())
    for u in range(updates):
        opt.zero_grad()
        for x, y in data[u * micro:(u + 1) * micro]:
            step(net, dev(net, x), dev(net, y), lr)
            z = ref.forward(x, True)
            (torch.nn.functional.cross_entropy(z, torch.from_numpy(y.astype(np.int64))) / micro).backward()
        if clip:
            torch.nn.utils.clip_grad_norm_(ref.parameters(), clip)
        opt.step()
    close_per_tensor(net.get_params(), ref.params(), IN_SHAPE, LAYERS, rtol, f"{tag} parameters")
    close(net.get_bn_stats(), ref.bn_stats(), rtol, f"{tag} running statistics")
    net.close()


def test_momentum_sgd_against_torch():
    import torch
    _against_torch(lambda n: n.set_sgd(0.9, 5e-4, False), lambda p: (torch.optim.SGD(p, lr=LR, momentum=0.9, weight_decay=5e-4), LR, None), tag="momentum SGD")


def test_adamw_with_decay_on_gamma_and_beta_against_torch():
    """eps = 1e-4, not 1e-8: the bias of a convolution in front of batch normalisation has gradient ZERO in exact arithmetic (the mean is
    subtracted), so the device holds fp32 rounding noise there (1e-9) where float64 holds 1e-18, and Adam divides by sqrt(v) + eps: with
    1e-8 it would turn that noise into steps of a tenth of the rate on the device and none in the reference.  Every real gradient of the
    net is above 1e-3, so 1e-4 leaves Adam's normalisation in place for them.  A deliberate choice of the test's recipe, argued from the
    arithmetic; the bound stays the project's 4e-4 per tensor."""
    import torch
    lr, wd = 1e-2, 0.05
    _against_torch(lambda n: n.set_adam((0.9, 0.999), 1e-4, wd, True), lambda p: (torch.optim.AdamW(p, lr=lr, betas=(0.9, 0.999), eps=1e-4, weight_decay=wd), lr, None), tag="AdamW")
    # ... and the decay reached gamma and beta: without it they end elsewhere (one update of lr * wd * gamma = 5e-4 on gamma around 1)
    flat = random_params(np.random.default_rng(6), IN_SHAPE, LAYERS)
    (x, y), = _host_batches(1)
    ends = []
    for w in (wd, 0.0):
        net = make_net(BN_A, "fp32")
        net.set_params(flat)
        net.set_adam((0.9, 0.999), 1e-4, w, True)
        step(net, dev(net, x), dev(net, y), lr)
        ends.append(net.get_params())
        net.close()
    g1 = tensor_slices(IN_SHAPE, LAYERS)[1][0]
    assert np.allclose(ends[1][g1] - ends[0][g1], lr * wd * flat[g1], rtol=1e-3, atol=1e-7)


def test_clip_against_torch():
    import torch
    _against_torch(lambda n: n.set_clip(0.25), lambda p: (torch.optim.SGD(p, lr=LR), LR, 0.25), tag="clip 0.25")


def test_accumulate_two_takes_per_micro_batch_statistics():
    import torch
    _against_torch(lambda n: n.set_accumulate(2), lambda p: (torch.optim.SGD(p, lr=LR), LR, None), micro=2, tag="accumulate 2")


def test_ema_evaluation_uses_the_averaged_gamma_and_beta_with_the_live_statistics():
    import torch
    flat = random_params(np.random.default_rng(8), IN_SHAPE, LAYERS)
    net = make_net(BN_A, "fp32")
    net.set_params(flat)
    net.set_ema(0.5)
    data = _host_batches(3)
    for x, y in data:
        step(net, dev(net, x), dev(net, y), LR)
    x, y = data[0]
    xd = dev(net, x)
    live = net.get_params()
    with torch.cuda.stream(net.stream):
        ze, zl = net.predict_logits(xd, weights="ema"), net.predict_logits(xd, weights="live")
    net.synchronize()
    for params, z, tag in ((net.get_ema(), ze, "ema"), (net.get_params(), zl, "live")):
        ref = TorchNet(IN_SHAPE, LAYERS, params)
        ref.set_bn_stats(net.get_bn_stats())
        close(z.cpu().numpy(), ref.logits(x, train=False), 2e-4, f"evaluation logits on the {tag} parameters, live statistics")
    g1 = tensor_slices(IN_SHAPE, LAYERS)[1][0]
    assert np.abs(net.get_ema()[g1] - net.get_params()[g1]).max() > 1e-5 and np.abs((ze - zl).cpu().numpy()).max() > 1e-4
    assert same_bits(net.get_params(), live)               # (the live parameters are back)
    net.close()


def test_snapshot_and_restore_round_trip_gamma_and_beta():
    a, = twins(BN_A, "fp32", 1, sgd=(0.9, 0.0, False))
    bs = batches(a, BN_A, 3)
    step(a, *bs[0], LR)
    snap = a.snapshot()
    kept = _state(a)
    g1, be1 = tensor_slices(IN_SHAPE, LAYERS)[1]
    assert same_bits(snap.desc.section(snap.body_bytes(), "params")[g1], kept[0][g1])
    step(a, *bs[1], LR)
    assert not same_bits(a.get_params()[g1], kept[0][g1]) and not same_bits(a.get_params()[be1], kept[0][be1])
    a.load_state(snap)
    assert same_bits(a.get_params(), kept[0]) and same_bits(a.get_velocity(), kept[2])
    a.close()


def test_save_and_load_continue_bit_for_bit(tmp_path):
    from mercer_research_amd.convnet import ConvNet, read_state_file
    a, = twins(BN_A, "fp32", 1, sgd=(0.9, 5e-4, True))
    a.set_bn(0.2, 1e-4)
    bs = batches(a, BN_A, 4)
    for x, y in bs[:2]:
        step(a, x, y, LR)
    path = tmp_path / "bn.state"
    a.save(path, extra=b"loop state")
    b, extra = ConvNet.load(path, B)
    assert extra == b"loop state" and b.get_bn() == a.get_bn() and _same(_state(a), _state(b))
    for x, y in bs[2:]:
        step(a, x, y, LR)
        step(b, x, y, LR)
    assert _same(_state(a), _state(b))
    # load_state into an existing net takes the statistics off the blob too; no blob stays None
    a.save(path)
    c = make_net(BN_A, "fp32")
    assert c.load_state(path) is None and _same(_state(a), _state(c))
    assert read_state_file(open(path, "rb").read())[2][:8] == b"RCNXBNS1"
    _close(a, b, c)


def test_a_file_of_a_net_without_bn_is_what_it_was(tmp_path):
    """The caller's blob is written as it is, and no blob is no blob: the bytes are write_state_file's of the snapshot, as before."""
    from mercer_research_amd.convnet import read_state_file, write_state_file
    net = make_net(PLAIN_A, "fp32")
    net.init_params(1)
    for extra in (None, b"xyz"):
        path = tmp_path / "plain.state"
        net.save(path, extra=extra)
        data = open(path, "rb").read()
        snap = net.snapshot()
        assert data == write_state_file(snap.desc, snap.body_bytes(), extra)
        assert read_state_file(data)[2] == extra
    net.close()
