"""Builds librcn_hip.so (the C-ABI library of include/rcn_hip.h) for gfx950 with hipcc, in-tree.

    python -m mercer_research_amd.build [--force]
"""
from __future__ import annotations

import os
import subprocess
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(HERE, "csrc")
LIB = os.path.join(HERE, "librcn_hip.so")
SOURCES = ["rcn_hip_api.hip"]
DEPS = ["rcn_hip_api_shapes.ipp", "rcn_hip_api_dense_launch.ipp", "rcn_hip_api_xcd.ipp", "rcn_hip_api_p2p.ipp", "rcn_hip_api_params.ipp", "rcn_hip_api_operators.ipp", "rcn_hip_api_features.ipp", "rcn_hip_api_dense.ipp", "rcn_hip_api_dp.ipp", "rcn_hip_api_sets.ipp", "common.hpp", "dense.hpp", "dense_pipe.hpp", "dense_p2.hpp", "features.hpp", "ops.hpp", "dp_rccl.hpp", "serve.hpp", "dp_p2p.hpp", "dense_p2_dp.hpp", "dense_xcd.hpp", "dense_wide.hpp", os.path.join("..", "..", "include", "rcn_hip.h")]
# -ffp-contract=off: the reference (rustc) never fuses a*b+c; the operator kernels reproduce its f64 rounding.
FLAGS = ["-O3", "--offload-arch=gfx950", "-ffp-contract=off", "-fPIC", "-shared", "-std=c++17", "-Wno-unused-result",
         "-Wno-pass-failed"]


def hipcc() -> str:
    for cand in (os.environ.get("HIPCC"), "/opt/rocm/bin/hipcc", "hipcc"):
        if cand and (os.path.isabs(cand) and os.path.exists(cand) or not os.path.isabs(cand)):
            return cand
    return "hipcc"


def stale() -> bool:
    if not os.path.exists(LIB):
        return True
    t = os.path.getmtime(LIB)
    return any(os.path.getmtime(os.path.join(CSRC, f)) > t for f in SOURCES + DEPS)


LIBX = os.path.join(HERE, "librcn_hipx.so")          # Track X (trainable conv net; include/rcn_hipx.h)
LIBX_SRC = os.path.join(CSRC, "rcn_hipx_api.hip")
LIBX_DEPS = [LIBX_SRC, os.path.join(CSRC, "convnet.hpp"), os.path.join(CSRC, "convnet_bf16.hpp"), os.path.join(CSRC, "convnet_loss.hpp"), os.path.join(CSRC, "convnet_epoch.hpp"), os.path.join(CSRC, "convnet_metrics.hpp"),os.path.join(CSRC, "convnet_halo.hpp"), os.path.join(CSRC, "convnet_halo_bf16.hpp"), os.path.join(CSRC, "convnet_select.hpp"), os.path.join(CSRC, "convnet_sgd.hpp"), os.path.join(CSRC, "convnet_adam.hpp"), os.path.join(CSRC, "convnet_ema.hpp"), os.path.join(CSRC, "convnet_clip.hpp"), os.path.join(CSRC, "convnet_accum.hpp"), os.path.join(CSRC, "convnet_update.hpp"), os.path.join(CSRC, "convnet_dropout.hpp"), os.path.join(CSRC, "convnet_state.hpp"), os.path.join(CSRC, "rcn_hipx_api_update.ipp"), os.path.join(CSRC, "rcn_hipx_api_dropout.ipp"), os.path.join(CSRC, "rcn_hipx_api_state.ipp"), os.path.join(CSRC, "convnet_bn.hpp"), os.path.join(CSRC, "rcn_hipx_api_bn.ipp"), os.path.join(CSRC, "convnet_gap.hpp"), os.path.join(CSRC, "convnet_pw.hpp"), os.path.join(CSRC, "convnet_dw.hpp"), os.path.join(CSRC, "convnet_dw_s2.hpp"), os.path.join(CSRC, "convnet_kinds.hpp"), os.path.join(HERE, "..", "include", "rcn_hipx.h")]


def build_x(force: bool = False, verbose: bool = False) -> str:
    if not force and os.path.exists(LIBX) and all(os.path.getmtime(f) <= os.path.getmtime(LIBX) for f in LIBX_DEPS):
        return LIBX
    cmd = [hipcc(), "-O3", "--offload-arch=gfx950", "-fPIC", "-shared", "-std=c++17", "-Wno-unused-result", "-o", LIBX, LIBX_SRC]
    if verbose:
        print(" ".join(cmd), flush=True)
    subprocess.run(cmd, check=True)
    return LIBX


CLI = os.path.join(HERE, "rcn_hip_cli")
CLI_SRC = os.path.join(CSRC, "host", "rcn_main.cpp")
CLI_DEPS = [CLI_SRC, os.path.join(CSRC, "host", "rcn.hpp"), os.path.join(CSRC, "host", "formats.hpp")]


def build_cli(force: bool = False, verbose: bool = False) -> str:
    """The C++ host side: rcn_hip_cli = rcn/src/main.rs over the C ABI (plain g++, links librcn_hip.so and zlib)."""
    if not force and os.path.exists(CLI) and all(os.path.getmtime(f) <= os.path.getmtime(CLI) for f in CLI_DEPS + [LIB]):
        return CLI
    cmd = ["g++", "-std=c++17", "-O2", "-Wall", CLI_SRC, "-L" + HERE, "-lrcn_hip", "-lz", "-Wl,-rpath,$ORIGIN", "-o", CLI]
    if verbose:
        print(" ".join(cmd), flush=True)
    subprocess.run(cmd, check=True)
    return CLI


def build(force: bool = False, verbose: bool = False) -> str:
    if force or stale():
        cmd = [hipcc()] + FLAGS + ["-o", LIB] + [os.path.join(CSRC, s) for s in SOURCES]
        if verbose:
            print(" ".join(cmd), flush=True)
        subprocess.run(cmd, check=True)
    build_cli(force, verbose)
    build_x(force, verbose)
    return LIB


if __name__ == "__main__":
    print(build(force="--force" in sys.argv, verbose=True))
