#!/usr/bin/env python3
"""Print tests/_kinds_cases.py's NUDGES anew: per wide tall-band net the (bn_relu layer, channel): k whose beta is moved by k * 1e-5 so that
no ReLU pre-activation of the float64 twin's training forward lies within 2e-6 of zero (the rule the CPU file asserts is 1e-6).

    python tools/kinds_nudges.py            # paste the output over NUDGES in tests/_kinds_cases.py

The loop, from the twin alone: on the parameters and the batch of SEEDS, every channel of either ReLU map that holds such a pre-activation
gets one more step; repeat until there is none.  A depthwise net keeps its channels apart, so a step moves that channel only (and the same
channel of the map above it)."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
NEAR = 2e-6


def near_zero(K, name, flat, x):
    """[(bn_relu layer, channel)] with a pre-activation within NEAR of zero, and the smallest |pre-activation| per ReLU map"""
    import torch
    in_shape, layers, _ = K.NETS[name]
    net = K.twin(name, "fp32", flat)
    found, smallest = [], []
    with torch.no_grad():
        net.forward(x, True)
        for i, l in enumerate(layers):
            if l == K.BNR:
                low = net.mods[i](net.outs[i - 1]).abs().amin((0, 2, 3)).numpy()
                smallest.append(float(low.min()))
                found += [(i, int(c)) for c in np.nonzero(low <= NEAR)[0]]
    return found, smallest


def main():
    import _kinds_cases as K
    print("NUDGES = {")
    for name in K.NUDGES:
        K.NUDGES[name] = {}
        for rounds in range(1, 40):
            flat, x, _ = K.case(name)
            found, smallest = near_zero(K, name, flat, x)
            print(f"{name} round {rounds}: {len(found)} channels, smallest |pre-activation| per map {smallest}", file=sys.stderr)
            if not found:
                break
            for key in found:
                K.NUDGES[name][key] = K.NUDGES[name].get(key, 0) + 1
        items, lines, cur = [f"({l}, {c}): {k}" for (l, c), k in sorted(K.NUDGES[name].items())], [], "        "
        for it in items:
            if len(cur) + len(it) > 150:
                lines.append(cur.rstrip())
                cur = "        "
            cur += it + ", "
        print(f'    "{name}": {{\n' + "\n".join(lines + [cur.rstrip()]) + "\n    },")
    print("}")


if __name__ == "__main__":
    main()
