"""CPU proof that tests/test_gpu_convnet_forms.py reaches what it claims: for every case of tests/_forms_cases.py the plan (rcn_hipx_plan:
the step's own dispatch code with every launch replaced by a note; options seeded from RCN_HIPX_* as at a net's creation) names the
promised kernel forms, every looping launch of a LOOPS case has at least two items per workgroup at every forced grid size, and the chunk
counts of the WGRADS cases are below the layers' pixel-block counts with one chunk shorter than the rest.  No GPU needed, none touched."""
import re

import pytest
from _convnet_util import convnet_built, plan_lines  # noqa: F401  (convnet_built: the fixture `convnet`)
from _forms_cases import CASES, LOOPS, OPTIONS, SLOTS, WGRADS, env_name, names

def plan_of(convnet, monkeypatch, case, options=None):
    for name, value in (case.options if options is None else options).items():
        monkeypatch.setenv(env_name(name), str(value))
    in_shape, layers, B = case.spec
    return plan_lines(convnet.plan(in_shape, layers, B, precision=case.precision, tiling=case.tiling))


def test_case_ids_are_unique_and_every_option_exists():
    from mercer_research_amd import convnet
    assert len({c.id for c in CASES}) == len(CASES)
    header = open(convnet.HERE + "/csrc/convnet_select.hpp").read()
    for c in CASES:
        for name in list(c.options) + list(c.twin or {}):
            assert f'{{"{name}", "{env_name(name)}"' in header, name


@pytest.mark.parametrize("case", CASES, ids=[c.id for c in CASES])
def test_the_plan_names_the_promised_kernel_forms(convnet, monkeypatch, case):
    L = plan_of(convnet, monkeypatch, case)
    for text in case.lines:
        assert any(names(l, text) for l in L), (text, L)


@pytest.mark.parametrize("case", LOOPS, ids=[c.id for c in LOOPS])
def test_every_looping_launch_has_two_items_per_workgroup_at_every_forced_grid(convnet, monkeypatch, case):
    """... and fewer items than the chip has slots: unforced, the same launches run one item per workgroup.  The looping kernels keep at
    least two workgroups on a compute unit (amdgpu_waves_per_eu of 2 or more on four-wave workgroups), and the chip has 256 of them: 512
    slots at the least (bf16-pipelined-3-column-blocks has 264 items; the other cases stay below 128)"""
    L = plan_of(convnet, monkeypatch, case)
    items = [(int(m.group(1)), l) for l in L for m in [re.search(r", (\d+) items", l)] if m]
    assert len(items) >= 2, L
    for n, l in items:
        assert 2 * max(SLOTS) <= n <= (264 if case.id == "bf16-pipelined-3-column-blocks" else 128), l
    # the forced grid is no part of the selection: the plan is the same at every slot count
    for s in SLOTS:
        assert plan_of(convnet, monkeypatch, case, dict(case.options, halo_f32_slots=s)) == L


def pixel_blocks(line):
    """(pixel blocks, chunks) of a weight-gradient line of the LDS-tiled kernels, from its shape, its kernel's block geometry and the batch
    in the plan's heading: 8 x 16 blocks of one image, or 8 x 8 blocks of two images side by side (k_wgrad3x3_halo_f32<8>, k_conv1_*<., 8>)"""
    m = re.search(r"wgrad conv3x3 (\d+)x(\d+)x\d+->\d+(?: pooled-dZ)?: (k_\w+)<([\d, ]+)>, (\d+) chunks", line)
    H, W, kernel, targs, chunks = int(m.group(1)), int(m.group(2)), m.group(3), [int(t) for t in m.group(4).split(",")], int(m.group(5))
    tw = 16 if kernel == "k_wgrad3x3_halo_bf16" else targs[-1]
    return lambda B: ((W + tw - 1) // tw) * ((H + 7) // 8) * ((B + 16 // tw - 1) // (16 // tw)), chunks


@pytest.mark.parametrize("case", WGRADS, ids=[c.id for c in WGRADS])
def test_weight_gradient_chunks_hold_several_pixel_blocks(convnet, monkeypatch, case):
    L = plan_of(convnet, monkeypatch, case)
    ragged = False
    for text in case.lines:
        if "wgrad" not in text and "k_wgrad" not in text and "k_conv1_wgrad" not in text:
            continue
        line = next(l for l in L if names(l, text))
        blocks_of, chunks = pixel_blocks(line)
        blocks = blocks_of(case.spec[2])
        # every chunk size that gives this chunk count (the plan prints the count, not the size)
        sizes = [b for b in range(1, blocks + 1) if (blocks + b - 1) // b == chunks]
        assert chunks < blocks and sizes and min(sizes) >= 2, (line, blocks, sizes)
        ragged = ragged or all(blocks % b for b in sizes)
    assert ragged or case.id.endswith("one-chunk"), L


@pytest.mark.parametrize("case", [c for c in OPTIONS if c.twin], ids=[c.id for c in OPTIONS if c.twin])
def test_a_twin_differs_in_the_schedule_only(convnet, monkeypatch, case):
    """what the GPU test compares bit for bit: same chunk counts, same kernels but for the form under test"""
    a = plan_of(convnet, monkeypatch, case)
    b = plan_of(convnet, monkeypatch, case, case.twin)
    assert len(a) == len(b)
    strip = lambda l: re.sub(r"k_conv3x3_halo_bf16\w*(<32>)?(, \d+ items)?", "k_conv3x3_halo_bf16*", l)
    assert [strip(l) for l in a] == [strip(l) for l in b]
    if "xcd_remap" in case.options:
        assert a == b                                          # the block order is no part of the plan
    else:
        assert a != b
