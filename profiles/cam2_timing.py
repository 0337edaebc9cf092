"""Cost of the explain entries on one MI355X: genconvit fp16 (ConvNeXt-T), the plain forward against explain at the last
stage (layer 3) and at the output of stage 2 (layer 2, csrc/cam_bwd.h), B = 15 and 128, alternating rounds on one box.
Also the workspace arena of the two handles, and the per-launch times of one profiled layer-2 call at B = 128.

    python profiles/cam2_timing.py [--steps 30] [--rounds 3] [--out profiles/cam2_timing.json]

Synthetic weights (genconvit_amd.synth), random frames; prints one JSON object and writes it to --out."""
from __future__ import annotations

import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from genconvit_amd import _lib, spec, synth                                  # noqa: E402


def handles(dtype, max_batch):
    he, hv = _lib.Handle(0, dtype, max_batch), _lib.Handle(0, dtype, max_batch)
    he.load_ed(synth.make_state_dict(spec.ed_spec(), synth.DEFAULT_SEED, "ed/"))
    hv.load_vae(synth.make_state_dict(spec.vae_spec(), synth.DEFAULT_SEED, "vae/"), with_var=False)
    return he, hv


def time_call(call, steps):
    for _ in range(3):
        call()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(steps):
        call()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / steps


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=30)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--out", default="profiles/cam2_timing.json")
    a = ap.parse_args()
    torch.set_grad_enabled(False)
    dtype = torch.float16
    he, hv = handles(dtype, 128)
    res = {"arena_bytes": {"ed": he.workspace_bytes(), "vae": hv.workspace_bytes()},
           "genconvit_fp16_ms": {str(B): {"forward": [], "layer3": [], "layer2": []} for B in (15, 128)}}
    data = {B: (torch.randn((B, 3, 224, 224), device="cuda").to(dtype), torch.randn((B, 12544), device="cuda"))
            for B in (15, 128)}
    for _ in range(a.rounds):                 # alternating batch sizes and entries
        for B in (15, 128):
            x, eps = data[B]
            calls = {"forward": lambda: _lib.genconvit_forward(he, hv, x, eps),
                     "layer3": lambda: _lib.genconvit_explain(he, hv, x, eps),
                     "layer2": lambda: _lib.genconvit_explain(he, hv, x, eps, layer="s2")}
            for k, call in calls.items():
                res["genconvit_fp16_ms"][str(B)][k].append(round(time_call(call, a.steps), 3))
    # where the layer-2 time goes: one profiled ED call at B = 128 (serial per-launch times), summed per tag
    x, eps = data[128]
    he.profile_enable(True)
    he.ed_explain(x, layer="s2")
    torch.cuda.synchronize()
    tags = {r["tag"]: {"launches": r["launches"], "ms": round(r["ms"], 4)} for r in he.profile_report()
            if r["tag"].startswith("explain")}
    he.profile_enable(False)
    res["ed_b128_explain_launches"] = tags
    print(json.dumps(res))
    os.makedirs(os.path.dirname(a.out) or ".", exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
