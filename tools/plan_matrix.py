"""The text (or the error) of rcn_hipx_plan / rcn_hipx_plan_buckets / rcn_hipx_plan_eval over a matrix of nets, batches, precisions, tilings and options, in a
fixed order.  No GPU needed.  Two builds choose the same kernels for every layer exactly when their outputs are equal:

    python tools/plan_matrix.py > after.txt          # and the same in a checkout of the commit to compare with (--root)
    diff before.txt after.txt

The output is not committed: it would pin every intended change of a dispatch rule.
"""
from __future__ import annotations

import argparse
import os
import sys

CONV_TAIL = (("dense_relu", 128), ("dense", 10))
# small nets that reach the branches the benchmark nets do not (name -> (input shape, layers))
# (the nets of the layer kinds that came after it -- batch normalisation, skips, global average pooling, stride 2, 1x1, depthwise -- are the
# tests' own: main() imports them)
SMALL = {
    # maps too small for the LDS-tiled weight gradient: bf16 storage refuses this one
    "w8": ((8, 8, 3), (("conv", 32), ("pool",), ("conv", 64), ("pool",), ("dense", 10))),
    "w12": ((12, 12, 3), (("conv", 32), ("pool",), ("conv", 64), ("pool",)) + CONV_TAIL),
    "w14": ((14, 14, 3), (("conv", 32), ("pool",), ("conv", 32), ("dense", 10))),
    "w24": ((24, 24, 3), (("conv", 32), ("pool",), ("conv", 64), ("pool",), ("conv", 128), ("pool",), ("dense_relu", 256), ("dense", 10))),
    "w56": ((56, 56, 3), (("conv", 32), ("conv", 32), ("pool",), ("conv", 64), ("pool",), ("dense", 10))),
    # a third convolution on the 7 x 7 map of the mnist shape (odd sides: no pool can follow)
    "odd7": ((28, 28, 1), (("conv", 32), ("pool",), ("conv", 64), ("pool",), ("conv", 64)) + CONV_TAIL),
    # two input channels: the gather loader without the first layer's own kernels
    "cin2": ((16, 16, 2), (("conv", 32), ("pool",), ("conv", 64), ("pool",), ("dense_relu", 64), ("dense", 10))),
    # channel pairs 32->32, 32->64, 64->128; convolutions in a row and one with no pool behind it
    "pairs": ((16, 16, 3), (("conv", 32), ("conv", 32), ("pool",), ("conv", 64), ("pool",), ("conv", 128)) + CONV_TAIL),
    # 96->96, and a hidden layer of 512 (no fused head)
    "c96": ((16, 16, 3), (("conv", 96), ("conv", 96), ("pool",), ("dense_relu", 512), ("dense", 10))),
    # 128->256, and no hidden dense layer (no fused head)
    "c256": ((16, 16, 1), (("conv", 128), ("conv", 256), ("pool",), ("dense", 10))),
    # refused by the layer table
    "bad_c48": ((16, 16, 3), (("conv", 48), ("pool",), ("dense", 10))),
    "bad_cin4": ((16, 16, 4), (("conv", 32), ("pool",), ("dense", 10))),
    "bad_oddpool": ((7, 7, 1), (("conv", 32), ("pool",), ("dense", 10))),
}
# Descriptions that break TWO rules (input shape, layers): which refusal wins is part of the interface.  A bias-only kind that names its
# layer is refused for what follows it before that layer's own checks run; plain conv_linear after them.
S2, PW, DW = "conv_linear_s2", "conv1x1_linear", "dwconv_linear"
PRECEDENCE = [
    # ... followed by a pool on an odd map, and by a convolution of 48 channels
    *[((6, 6, 32) if kind == S2 else (3, 3, 32), ((kind, 32), ("pool",), ("dense", 4))) for kind in (S2, PW, DW, "conv_linear")],
    *[((4, 4, 32), ((kind, 32), ("conv", 48), ("dense", 4))) for kind in (S2, PW, DW, "conv_linear")],
    *[((4, 4, 32), ((kind, 32), ("dense", 4))) for kind in (S2, PW, DW, "conv_linear")],
    # ... as the last layer
    *[((4, 4, 32), (("conv", 32), (kind, 32))) for kind in (S2, PW, DW, "conv_linear")],
    # a depthwise layer with a bad `out` behind a dense layer, and on a map
    ((4, 4, 32), (("conv", 32), ("dense_relu", 32), (DW, 48), ("bn_relu",), ("dense", 4))),
    ((4, 4, 32), (("conv", 32), (DW, 48), ("bn_relu",), ("dense", 4))),
    # a strided layer: 48 input channels on an odd map, 3 input channels on an odd map, 48 output channels behind a dense layer
    ((5, 5, 48), ((S2, 32), ("bn_relu",), ("dense", 4))),
    ((5, 5, 3), ((S2, 32), ("bn_relu",), ("dense", 4))),
    ((4, 4, 32), (("conv", 32), ("dense_relu", 32), (S2, 48), ("bn_relu",), ("dense", 4))),
    # a 1x1 layer: 48 output channels on 3 input channels
    ((4, 4, 3), ((PW, 48), ("bn_relu",), ("dense", 4))),
]
BATCHES = (1, 2, 7, 16, 128, 512, 4096)
PRECISIONS = ("fp32", "bf16", "bf16_stored")
TILINGS = ("gemm", "auto", "lds")
# one at a time, through the environment (a plan seeds its options from it on every call)
OPTIONS = (("HALO", 0), ("BF16_PIPE", 0), ("BF16_1CB", 0), ("BF16_ROWS16", 1), ("HALO_WGRAD", 0), ("FUSE_POOL_BWD", 0), ("HEAD", 0), ("XCD_REMAP", 1),
           ("PIX_PER_CHUNK", 256), ("WG_TARGET", 1024), ("WGH_F32_TARGET", 128), ("WGH_TARGET", 512), ("WGB_POLICY", 0), ("WGF_POLICY", 0))
BUCKETS = (0, 256 << 10, 1 << 20, 1 << 30)


def main() -> None:
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--root", default=os.path.dirname(os.path.dirname(os.path.abspath(__file__))), help="the checkout whose built library is asked (default: this one)")
    root = os.path.abspath(ap.parse_args().root)
    sys.path[:0] = [root, os.path.join(root, "tests")]
    import bench_convnet as bc
    import _dw_ref, _kinds_cases, _mb_ref, _pw_ref, _stride_ref    # the twins' nets, and every description the plan tests expect refused
    import test_convnet_bn_plan as bn, test_convnet_dw_plan as dw, test_convnet_gap_plan as gap, test_convnet_mb_plan as mb, test_convnet_pw_plan as pw, test_convnet_res_plan as res, test_convnet_stride_plan as stride
    from mercer_research_amd.convnet import ConvNetError, plan, plan_eval
    for k in list(os.environ):
        if k.startswith("RCN_HIPX_"):
            del os.environ[k]

    def show(title, in_shape, layers, batch, **kw):
        # the training step (or its bucketed gradient walk), then -- where it is a step -- one evaluation chunk of the same net
        for what, fn in (("", plan), (" eval", plan_eval)) if "buckets" not in kw else (("", plan),):
            print(f"==== {title}{what}")
            try:
                print("status 0\n" + fn(in_shape, layers, batch, **kw))
            except ConvNetError as e:
                print(e)

    nets = [(name, shape, layers, tuple(b for b in BATCHES if b <= 128) if name == "synth224" else BATCHES) for name, (shape, layers, _) in bc.CONFIGS.items()]
    nets += [(name, shape, layers, BATCHES) for name, (shape, layers) in SMALL.items()]
    # the nets of the newer kinds' tests (input shape, layers, the test's own batch): at that batch and at the batches above
    for tag, group in (("stride", _stride_ref.NETS), ("pw", _pw_ref.NETS), ("dw", _dw_ref.NETS), ("mb", _mb_ref.NETS), ("kinds", {**_kinds_cases.NETS, **{"X" + k: v for k, v in _kinds_cases.EXACT.items()}}),
                       ("bn", bn.BN_NETS), ("res", res.RES_NETS), ("gap", gap.GAP_NETS)):
        nets += [(f"{tag}_{name}", shape, layers, tuple(sorted({b0, *BATCHES}))) for name, (shape, layers, b0) in group.items()]
    for name, shape, layers, batches in nets:
        for b in batches:
            for p in PRECISIONS:
                for t in TILINGS:
                    show(f"{name} B={b} {p} {t}", shape, layers, b, precision=p, tiling=t)
    # the runs of tests/_kinds_cases.py under their own options (pw, halo_f32_slots, wg_target), which the matrix above leaves at their defaults
    for name, p, options in _kinds_cases.RUNS + [("X" + n, p, o) for n, o in _kinds_cases.EXACT_RUNS for p in ("fp32", "bf16")]:
        if options:
            shape, layers, b0 = _kinds_cases.EXACT[name[1:]] if name[0] == "X" else _kinds_cases.NETS[name]
            os.environ.update({"RCN_HIPX_" + k.upper(): str(v) for k, v in options})
            show(f"kinds_{name} B={b0} {p} auto " + " ".join(f"RCN_HIPX_{k.upper()}={v}" for k, v in options), shape, layers, b0, precision=p)
            for k, _ in options:
                del os.environ["RCN_HIPX_" + k.upper()]
    refused = [(r[0], r[1]) for m in (stride, pw, dw, mb) for r in m.REFUSALS] + [((4, 4, 32), r[0]) for m in (res, gap) for r in m.REFUSALS] + PRECEDENCE
    for k, (shape, layers) in enumerate(refused):
        show(f"refusal {k}: {shape} {layers}", shape, layers, 2)
    for env, value in OPTIONS:
        os.environ["RCN_HIPX_" + env] = str(value)
        for name, (shape, layers, b0) in bc.CONFIGS.items():
            for b in (16, b0):
                for p in PRECISIONS:
                    show(f"{name} B={b} {p} auto RCN_HIPX_{env}={value}", shape, layers, b, precision=p)
        del os.environ["RCN_HIPX_" + env]
    for name, (shape, layers, b0) in bc.CONFIGS.items():
        for p in PRECISIONS:
            for nbytes in BUCKETS:
                show(f"{name} B={b0} {p} auto buckets>={nbytes}", shape, layers, b0, precision=p, buckets=nbytes)


if __name__ == "__main__":
    main()
