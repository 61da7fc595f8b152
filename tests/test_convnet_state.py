"""CPU side of Track X's save and resume (include/rcn_hipx.h: rcn_hipx_state_desc, rcn_hipx_state_layout, rcn_hipx_snapshot_dev,
rcn_hipx_restore_dev, rcn_hipx_set_accumulated): the names are declared, exported and bound; the descriptor has one size on both sides;
the layout of a body agrees with the oracle's parameter shapes; the file codec round-trips and refuses damaged files; NULL arguments are
refused.  None of it needs a GPU."""
import ctypes as C
import re

import numpy as np
import pytest
from _convnet_util import FUSED_HEAD, HEADER, ODD_WIDTH, PLAIN_HEAD, convnet_loaded  # noqa: F401  (fixture `convnet`)

from oracle import convnet_oracle as co

NEW = ("rcn_hipx_state_desc_size", "rcn_hipx_state_layout", "rcn_hipx_snapshot_dev", "rcn_hipx_restore_dev", "rcn_hipx_set_accumulated")
ALL = ("params", "velocity", "adam_m", "adam_v", "ema", "accum")


def test_names_are_declared_exported_and_bound(convnet):
    text = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    declared = set(re.findall(r"\b(rcn_hipx_[a-z0-9_]+)\s*\(", text))
    raw = C.CDLL(convnet.LIBX_PATH)
    for name in NEW:
        assert name in declared, name
        assert hasattr(raw, name), name
        assert name in convnet.SIGNATURES, name
    assert "typedef struct rcn_hipx_state_desc" in text
    # the constants the binding restates are the header's
    for macro, value in (("RCN_HIPX_STATE_MAGIC", convnet.STATE_MAGIC), ("RCN_HIPX_STATE_VERSION", convnet.STATE_VERSION),
                         ("RCN_HIPX_STATE_MAX_LAYERS", convnet.STATE_MAX_LAYERS), ("RCN_HIPX_STATE_SECTIONS", convnet.STATE_SECTIONS)):
        m = re.search(r"#define\s+%s\s+(0x[0-9a-fA-F]+|\d+)u?" % macro, text)
        assert m and int(m.group(1), 0) == value, macro
    for name, bit in convnet.SECTIONS.items():
        assert bit in (1, 2, 4, 8, 16, 32), name
    assert len(convnet.SECTIONS) == convnet.STATE_SECTIONS


def test_descriptor_size_is_the_c_side(convnet):
    lib = convnet.load()
    assert C.sizeof(convnet.StateDesc) == lib.rcn_hipx_state_desc_size() == 688


@pytest.mark.parametrize("spec", [FUSED_HEAD, PLAIN_HEAD, ODD_WIDTH], ids=["fused_head", "plain_head", "odd_width"])
@pytest.mark.parametrize("sections", [("params",), ALL, ("params", "adam_m", "accum")], ids=["model", "all", "some"])
def test_layout_agrees_with_the_oracle(convnet, spec, sections):
    in_shape, layers, _ = spec
    d = convnet.state_layout(in_shape, layers, sections)
    shapes = co.param_shapes(in_shape, layers)
    n_log = sum(int(np.prod(k)) + int(n) for k, n in shapes)
    assert d.magic == convnet.STATE_MAGIC and d.version == convnet.STATE_VERSION
    assert (d.in_h, d.in_w, d.in_c) == tuple(in_shape) and d.n_layers == len(layers) and d.classes == layers[-1][1]
    assert d.shape_and_layers() == (tuple(in_shape), [tuple(l) for l in layers])
    assert d.n_log == n_log
    # per layer: W at layer_off, b behind it, the next layer behind that; pools have none
    at, with_params = 0, iter(shapes)
    for i, l in enumerate(layers):
        if l[0] == "pool":
            assert d.layer_off[i] == -1
            continue
        k, n = next(with_params)
        assert d.layer_off[i] == at, (i, d.layer_off[i], at)
        at += int(np.prod(k)) + int(n)
    assert at == n_log and all(d.layer_off[i] == -1 for i in range(len(layers), convnet.STATE_MAX_LAYERS))
    # sections: 256-byte aligned, in order, not overlapping, behind the scalars block; body_bytes as computed
    want = sum(convnet.SECTIONS[s] for s in sections)
    assert d.sections == want
    end = convnet.STATE_SCALARS_BYTES
    for s in range(convnet.STATE_SECTIONS):
        if not want >> s & 1:
            assert d.section_off[s] == -1
            continue
        assert d.section_off[s] % 256 == 0 and d.section_off[s] == end, (s, d.section_off[s], end)
        end = d.section_off[s] + (4 * n_log + 255) // 256 * 256
    assert d.body_bytes == end == 256 + len(sections) * ((4 * n_log + 255) // 256 * 256)
    # the recipe at its defaults
    assert (d.flags, d.accum_pos, d.optim, d.accum_k, d.sgd_momentum, d.ema_decay, d.clip_max_norm, d.dropout_p, d.loss_eps) == (0, 0, 0, 1, 0, 0, 0, 0, 0)
    assert (d.adam_beta1, d.adam_beta2, d.adam_eps) == (np.float32(0.9), np.float32(0.999), np.float32(1e-8))


def test_layout_refusals(convnet):
    lib = convnet.load()
    in_shape, layers, _ = FUSED_HEAD
    arr, d = convnet._layer_array(layers), convnet.StateDesc()
    ok = (in_shape[0], in_shape[1], in_shape[2], arr, len(layers), 1)
    assert lib.rcn_hipx_state_layout(*ok, C.byref(d)) == 0
    assert lib.rcn_hipx_state_layout(*ok, None) == -1
    assert lib.rcn_hipx_state_layout(in_shape[0], in_shape[1], in_shape[2], None, len(layers), 1, C.byref(d)) == -1
    assert lib.rcn_hipx_state_layout(0, in_shape[1], in_shape[2], arr, len(layers), 1, C.byref(d)) == -1
    assert lib.rcn_hipx_state_layout(in_shape[0], in_shape[1], in_shape[2], arr, len(layers), 64, C.byref(d)) == -1      # an unknown section bit
    deep = [("conv", 32)] * 33 + [("dense", 10)]
    assert lib.rcn_hipx_state_layout(8, 8, 3, convnet._layer_array(deep), len(deep), 1, C.byref(d)) == -3
    with pytest.raises(convnet.ConvNetError):
        convnet.state_layout((8, 8, 3), (("conv", 32), ("pool",)), ("params",))                                          # no logits layer


def test_null_arguments_and_a_misaligned_body_are_refused(convnet):
    lib = convnet.load()
    d = convnet.state_layout(FUSED_HEAD[0], FUSED_HEAD[1])
    flat = np.zeros(int(d.n_log), dtype=np.float32)
    aligned, misaligned = C.c_void_p(4096), C.c_void_p(4096 + 4)
    assert lib.rcn_hipx_snapshot_dev(None, 0, aligned, d.body_bytes, C.byref(d)) == -1
    assert lib.rcn_hipx_snapshot_dev(None, 0, misaligned, d.body_bytes, C.byref(d)) == -1
    assert lib.rcn_hipx_restore_dev(None, C.byref(d), aligned, d.body_bytes) == -1
    assert lib.rcn_hipx_restore_dev(None, C.byref(d), misaligned, d.body_bytes) == -1
    assert lib.rcn_hipx_restore_dev(None, None, None, 0) == -1
    assert lib.rcn_hipx_set_accumulated(None, flat.ctypes.data_as(C.POINTER(C.c_float)), 0) == -1


def _synthetic(convnet, sections=ALL):
    d = convnet.state_layout(PLAIN_HEAD[0], PLAIN_HEAD[1], sections)
    d.flags, d.optim, d.accum_k, d.accum_pos, d.dropout_seed = 15, 1, 3, 1, 2 ** 63 + 5
    body = np.random.default_rng(7).integers(0, 256, int(d.body_bytes)).astype(np.uint8)
    return d, body


@pytest.mark.parametrize("extra", [None, b"", b"epoch 3, next batch 17, permutation seed 5\x00\xff"], ids=["none", "empty", "blob"])
def test_file_codec_round_trip(convnet, extra):
    d, body = _synthetic(convnet)
    data = convnet.write_state_file(d, body, extra)
    assert data[:8] == convnet.STATE_FILE_MAGIC
    assert len(data) == 8 + 4 + 8 + 8 + C.sizeof(convnet.StateDesc) + body.size + len(extra or b"") + 4
    d2, body2, extra2 = convnet.read_state_file(data)
    assert bytes(d2) == bytes(d) and np.array_equal(body2, body) and body2.dtype == np.uint8
    assert extra2 == (extra or None)
    assert (d2.accum_k, d2.accum_pos, d2.dropout_seed, d2.flags) == (3, 1, 2 ** 63 + 5, 15)
    # a section of the body as floats, by name
    s = convnet.SECTIONS["ema"].bit_length() - 1
    assert d2.section(body2, "ema").tobytes() == body[int(d.section_off[s]):int(d.section_off[s]) + 4 * int(d.n_log)].tobytes()
    assert convnet.write_state_file(d2, body2, extra2) == data


def test_damaged_files_are_refused(convnet):
    d, body = _synthetic(convnet, ("params",))
    data = convnet.write_state_file(d, body, b"x")
    convnet.read_state_file(data)
    head = 8 + 4 + 8 + 8
    flipped = bytearray(data)
    flipped[head + C.sizeof(convnet.StateDesc) + 100] ^= 0x10                   # one bit of the body
    magic = b"RCNXSTA0" + data[8:]
    for bad in (data[:-1], data[:len(data) // 2], data[:10], b"", bytes(flipped), magic, data + b"\x00"):
        with pytest.raises(convnet.ConvNetError):
            convnet.read_state_file(bad)
    with pytest.raises(convnet.ConvNetError):
        convnet.write_state_file(d, body[:-1])                                  # a body that is not the descriptor's
