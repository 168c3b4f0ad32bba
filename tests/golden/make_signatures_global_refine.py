#!/usr/bin/env python3
"""Record the INTERFACE of the reference's dense global-alignment package as data (tests/golden/signatures_global_refine.json):
the call signatures of what run_global_refine.py / eval_sintel_depth.py / eval_shibuya_depth.py import from `model.*` —
RefineNet.__init__, global_alignment_loop, the two lr schedules, eval_depth, eval_depth_metric and compute_errors.  Run in
the build container only (needs the reference checkout), with the pypose stand-in.  Names and signature strings only.

    python tests/golden/make_signatures_global_refine.py
"""
import inspect
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
REF = "/root/reference/main/global_refine"
sys.path[:0] = [os.path.join(HERE, "refstubs"), REF]

from model import refine_net, trainer, utils       # noqa: E402  (reference, unmodified)

sig = lambda f: str(inspect.signature(f))
out = {
    "source": "wrchen530/batrack main/global_refine/model (signatures only)",
    "refine_net": {"RefineNet.__init__": sig(refine_net.RefineNet.__init__)},
    "trainer": {n: sig(getattr(trainer, n)) for n in ("global_alignment_loop", "cosine_schedule", "linear_schedule")},
    "utils": {n: sig(getattr(utils, n)) for n in ("eval_depth", "eval_depth_metric", "compute_errors")},
    "script_imports": ["from model.refine_net import RefineNet", "from model.trainer import global_alignment_loop",
                       "from model.utils import eval_depth"],
}
json.dump(out, open(os.path.join(HERE, "signatures_global_refine.json"), "w"), indent=1, sort_keys=True)
print(json.dumps(out, indent=1))
