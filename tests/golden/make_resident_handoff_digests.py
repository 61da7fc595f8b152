#!/usr/bin/env python3
"""Pins what the resident one-XCD kernel (csrc/dense_xcd.hpp, dense path 5) computes, bit for bit: for every instantiation -- f32 and
f64, every batch tile (32 / 64 / 128 / 256), full and padded batches, one and two hidden layers, the data-parallel form at a group of
one -- the SHA-256 of the parameter bytes and of the per-step costs after 3 and after 130 steps (130 steps are three launches of at
most 64 steps), plus the first 16 values of each for diagnosis.

    python tests/golden/make_resident_handoff_digests.py [out.json]       (on the GPU; library API only)

Run on the commit whose results are the reference; tests/test_gpu_resident_handoff.py recomputes and compares.  A change to the
kernel that alters neither an operand nor an order of summation leaves every digest as it is.
"""
import hashlib
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
OUT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "resident_handoff_digests.json")

STEPS = (3, 130)
N_IMAGES = 130 * 256                                   # rows for 130 steps at the largest batch


def cases():
    out = []
    for nb in STEPS:
        for B in (10, 32, 64, 100, 128, 200, 256):
            out.append({"id": f"f32-784-30-10-B{B}-{nb}steps", "dtype": "f32", "hidden": [30], "B": B, "steps": nb, "dp": False})
        for B in (10, 32, 128, 256):
            out.append({"id": f"f64-784-30-10-B{B}-{nb}steps", "dtype": "f64", "hidden": [30], "B": B, "steps": nb, "dp": False})
        for B in (32, 256):
            out.append({"id": f"f32-784-10-10-10-B{B}-{nb}steps", "dtype": "f32", "hidden": [10, 10], "B": B, "steps": nb, "dp": False})
        out.append({"id": f"f32-784-30-10-B256-{nb}steps-data-parallel-world1", "dtype": "f32", "hidden": [30], "B": 256, "steps": nb, "dp": True})
    return out


_images = None


def _data():
    global _images
    if _images is None:
        from mercer_research_amd.synth import synthetic_images
        _images = synthetic_images(N_IMAGES, seed=1234)
    return _images


def run_case(case):
    """One case on a fresh context -> {"params_sha256", "loss_sha256", "params_head", "loss_head"}."""
    import torch
    import mercer_research_amd as amd
    from mercer_research_amd.device import DeviceRCN
    from mercer_research_amd.synth import synthetic_params
    imgs, labels = _data()
    dims = [784] + list(case["hidden"]) + [10]
    B, nb = case["B"], case["steps"]
    d = DeviceRCN(classes=10, feedforward_cfg=case["hidden"], input_shape=(28, 28), dtype=amd.F64 if case["dtype"] == "f64" else amd.F32)
    try:
        d.set_dense_path(5)                             # the resident kernel or an error: no other path can answer
        ws, bs = synthetic_params(dims, seed=42)
        d.set_params([w * 0.1 for w in ws], bs)
        with torch.cuda.stream(d.stream):
            imgs_d, labels_d = torch.from_numpy(imgs).to(d.device), torch.from_numpy(labels).to(d.device)
        X, Y = d.load_data(imgs_d, labels_d)
        perm = torch.empty(N_IMAGES, dtype=torch.int32, device=d.device)
        d.shuffle(perm, N_IMAGES, 1, seed=20240 + B)
        loss = d.empty(nb)
        if case["dp"]:
            d.set_option("dp_p2p", 2)                   # the peer exchange's bootstrap forced on at a group of one
            d.dp_init()                                 # (a one-rank communicator; an error here is an error of the case)
            assert d.dp_resident(B), "the data-parallel step does not run on the resident kernel here"
            d.dp_train_epoch(X, Y, perm, B, nb, 3.0, loss)
        else:
            assert d.train_epoch_resident(B)
            d.train_epoch(X, Y, perm, B, nb, 3.0, loss)
        d.synchronize()
        assert d.fallbacks_taken() == 0, "a launch stepped down to another path"
        p = d.params_flat().cpu().numpy()
        c = loss.cpu().numpy()
        if case["dp"]:
            d.dp_finalize()
    finally:
        d.rcn.close()
    return {"params_sha256": hashlib.sha256(p.tobytes()).hexdigest(), "loss_sha256": hashlib.sha256(c.tobytes()).hexdigest(),
            "params_head": [float(v).hex() for v in p[:16]], "loss_head": [float(v).hex() for v in c[:16]]}


def main():
    out = {}
    for case in cases():
        out[case["id"]] = run_case(case)
        print(case["id"], out[case["id"]]["params_sha256"][:16], out[case["id"]]["loss_sha256"][:16], flush=True)
    path = sys.argv[1] if len(sys.argv) > 1 else OUT
    with open(path, "w") as f:
        json.dump(out, f, indent=1, sort_keys=True)
        f.write("\n")
    print("wrote", path, len(out), "cases")


if __name__ == "__main__":
    main()
