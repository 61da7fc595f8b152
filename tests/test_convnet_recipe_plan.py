"""CPU tests of Track X's training recipe pieces that need no GPU (include/rcn_hipx.h): the augmentation's draw through
rcn_hipx_augment_draw -- the host side of the one function k_gather_aug runs -- against the header's known answers and a Python
restatement of the formula, the warm-up + cosine schedule, and the refusals of the new entry points.  rcn_hipx_plan_epoch_net walks an
EXISTING net, which only a GPU machine can create: its lines are held in tests/test_gpu_convnet_recipe.py."""
import ctypes as C

import numpy as np
import pytest
from _convnet_util import convnet_loaded  # noqa: F401  (the fixture `convnet`)
from _recipe_ref import M64, draw_ref


def _draws(convnet, pad, hflip, seed, epoch, q0, count):
    return [tuple(int(v) for v in row) for row in convnet.augment_draws(convnet.Augment(pad, hflip, seed, epoch), q0, count)]


def test_draw_returns_the_known_answers(convnet):
    assert _draws(convnet, 2, True, 7, 0, 0, 6) == [(-2, -1, 0), (-1, 2, 1), (-2, 1, 0), (-2, 0, 0), (-2, 0, 0), (1, 1, 0)]
    assert _draws(convnet, 2, True, 7, 1, 0, 3) == [(0, 0, 0), (0, 2, 0), (0, -1, 1)]
    assert _draws(convnet, 4, True, 0, 0, 0, 1) == [(3, 0, 1)]
    assert _draws(convnet, 8, True, M64, (1 << 32) + 5, (1 << 40) + 3, 1) == [(2, 2, 1)]
    for seed, epoch in ((0, 0), (7, 3), (M64, M64)):
        assert set(_draws(convnet, 0, False, seed, epoch, 0, 64)) == {(0, 0, 0)}
    # the restatement below gives them too: the two checks hold each other
    assert [draw_ref(7, 0, 2, 1, q) for q in range(6)] == _draws(convnet, 2, True, 7, 0, 0, 6)


@pytest.mark.parametrize("pad", [0, 1, 2, 4, 16])
def test_draw_is_the_formula_and_stays_in_range(convnet, pad):
    for seed in (7, 0xDEADBEEFCAFEF00D):
        for epoch in (0, 5):
            got = _draws(convnet, pad, True, seed, epoch, 0, 2048)
            assert got == [draw_ref(seed, epoch, pad, 1, q) for q in range(2048)]
            a = np.array(got)
            assert a[:, :2].min() >= -pad and a[:, :2].max() <= pad and set(a[:, 2]) <= {0, 1}
            noflip = _draws(convnet, pad, False, seed, epoch, 0, 2048)
            assert all(f == 0 for _, _, f in noflip)
            assert [d[:2] for d in noflip] == [d[:2] for d in got]      # the flip bit is its own bit: the translation does not depend on hflip


def test_draws_cover_every_outcome_and_change_with_the_epoch(convnet):
    e0 = _draws(convnet, 2, True, 7, 0, 0, 58)
    e1 = _draws(convnet, 2, True, 7, 1, 0, 58)
    assert {d[0] for d in e0} == {d[1] for d in e0} == {-2, -1, 0, 1, 2} and {d[2] for d in e0} == {0, 1}
    assert sum(a != b for a, b in zip(e0, e1)) == 56
    # a position's draw does not depend on where the call starts
    assert _draws(convnet, 2, True, 7, 0, 40, 18) == e0[40:]


def test_draw_refusals_without_a_gpu(convnet):
    lib = convnet.load()
    dy, dx, fl = C.c_int(9), C.c_int(9), C.c_int(9)
    out = (C.byref(dy), C.byref(dx), C.byref(fl))
    assert lib.rcn_hipx_augment_draw(None, 0, *out) == -1
    for pad, hflip in ((-1, 0), (17, 1), (2, 2), (2, -1)):
        a = convnet.AugmentStruct(pad, hflip, 0, 0)
        assert lib.rcn_hipx_augment_draw(C.byref(a), 0, *out) == -1
    assert (dy.value, dx.value, fl.value) == (9, 9, 9)
    a = convnet.AugmentStruct(16, 1, 3, 4)
    assert lib.rcn_hipx_augment_draw(C.byref(a), 5, None, None, None) == 0           # the outputs are nullable
    assert lib.rcn_hipx_augment_draw(C.byref(a), 5, *out) == 0 and (dy.value, dx.value, fl.value) == draw_ref(3, 4, 16, 1, 5)
    with pytest.raises(convnet.ConvNetError):
        convnet.augment_draws(convnet.Augment(pad=17), 0, 1)


def test_new_entry_points_refuse_null_nets_without_a_gpu(convnet):
    lib = convnet.load()
    a = convnet.AugmentStruct(2, 1, 0, 0)
    assert lib.rcn_hipx_train_epoch_ex_dev(None, None, 0, 1.0, 0.0, None, 1, None, 1, 0, 1, 0.1, None, C.byref(a), None) == -1
    assert lib.rcn_hipx_gather_batch_dev(None, None, 0, 1.0, 0.0, None, 1, None, 0, 1, C.byref(a), 0, None, None) == -1
    buf = C.create_string_buffer(b"untouched", 64)
    assert lib.rcn_hipx_plan_epoch_net(None, 1, 0, 0, None, buf, len(buf)) == -1 and buf.value == b"untouched"
    assert lib.rcn_hipx_plan_epoch_net(None, 1, 1, 1, C.byref(a), buf, len(buf)) == -1


def test_augment_struct_is_the_headers(convnet):
    assert C.sizeof(convnet.AugmentStruct) == 24
    s = convnet.Augment(pad=3, hflip=False, seed=-1, epoch=1 << 64).struct()         # masked to 64 bits
    assert (s.pad, s.hflip, s.seed, s.epoch) == (3, 0, M64, 0)
    assert convnet.Augment() == convnet.Augment(4, True, 0, 0)


def test_warmup_cosine(convnet):
    lr = convnet.warmup_cosine(100, 0.2, 10, floor=0.01)
    assert lr.dtype == np.float32 and lr.shape == (100,)
    assert lr[0] == np.float32(0.2 / 10) and lr[9] == np.float32(0.2) and lr[10] == np.float32(0.2) and lr[-1] == np.float32(0.01)
    assert np.all(np.diff(lr[:10].astype(np.float64)) > 0) and np.all(np.diff(lr[10:].astype(np.float64)) < 0)
    want = 0.01 + (0.2 - 0.01) * 0.5 * (1.0 + np.cos(np.pi * np.arange(90, dtype=np.float64) / 89))
    assert np.array_equal(lr[10:], want.astype(np.float32))
    assert np.array_equal(lr[:10], (0.2 * np.arange(1, 11, dtype=np.float64) / 10).astype(np.float32))
    # no warm-up, all warm-up, one step
    assert convnet.warmup_cosine(5, 1.0, 0)[0] == 1.0 and convnet.warmup_cosine(5, 1.0, 0)[-1] == 0.0
    assert np.array_equal(convnet.warmup_cosine(4, 1.0, 4), np.array([0.25, 0.5, 0.75, 1.0], dtype=np.float32))
    assert np.array_equal(convnet.warmup_cosine(1, 0.5, 0), np.array([0.5], dtype=np.float32))
    for bad in ((0, 1.0, 0), (4, 1.0, 5), (4, 1.0, -1)):
        with pytest.raises(ValueError):
            convnet.warmup_cosine(*bad)
