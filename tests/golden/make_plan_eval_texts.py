"""Records rcn_hipx_plan_eval's text (or its refusal) for the shared Track X specs in every precision into plan_eval_texts.json, which
tests/test_convnet_eval_metrics.py holds the plain evaluation plans to.  Needs no GPU.

    python tests/golden/make_plan_eval_texts.py

Run it on a tree whose evaluation plans are known to be right: the file was first recorded from the commit before k_eval_metrics existed.
"""
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path[:0] = [os.path.dirname(os.path.dirname(HERE)), os.path.dirname(HERE)]

from mercer_research_amd import convnet  # noqa: E402

from test_convnet_eval_metrics import PLAN_SPECS  # noqa: E402

out = {}
for name, (shp, layers, B) in PLAN_SPECS.items():
    for precision in ("fp32", "bf16", "bf16_stored"):
        try:
            out[f"{name}-{precision}"] = convnet.plan_eval(shp, layers, B, precision, "auto")
        except convnet.ConvNetError as e:
            out[f"{name}-{precision}"] = "refused: " + str(e)
with open(os.path.join(HERE, "plan_eval_texts.json"), "w") as f:
    json.dump(out, f, indent=1, sort_keys=True)
    f.write("\n")
print(len(out), "texts")
