"""Cost of gcv_track_match (csrc/follow.hip) on one MI355X beside the scoring it feeds.  One shape, the one a scan with
``follow=True`` meets on 720p footage: 1024 jobs on 8 frames of 720 x 1280, faces of about 200 pixels, grid 64,
radius 16.  Timed with HIP events, one pair per call, median over --steps calls after warm-up, in alternating rounds:
  match        one gcv_track_match launch through the C ABI, jobs already on the device
  match_r0     the same launch with radius 0: the prior's and the templates' cells and one candidate — phase 1 without
               the margin cells, next to nothing of phase 2
  score        the same 1024 boxes through _lib.face_crop_preprocess and the fp16 ensemble forward (synthetic weights), in
               groups of 128 as scan_frames runs them

    python profiles/follow_timing.py [--steps 20] [--rounds 3] [--out profiles/follow_timing.json]

Random frames; prints one JSON object and writes it to --out."""
from __future__ import annotations

import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from genconvit_amd import _lib, spec, synth                                  # noqa: E402
from genconvit_amd.model.config import load_config                           # noqa: E402
from genconvit_amd.model.genconvit import GenConViT                          # noqa: E402
from genconvit_amd.model.genconvit_ed import GenConViTED                     # noqa: E402
from genconvit_amd.model.genconvit_vae import GenConViTVAE                   # noqa: E402

NF, H, W, N, GRID, RADIUS, GROUP = 8, 720, 1280, 1024, 64, 16, 128


def median_ms(call, steps, warmup=3):
    for _ in range(warmup):
        call()
    torch.cuda.synchronize()
    ms = []
    for _ in range(steps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        call()
        e1.record()
        torch.cuda.synchronize()
        ms.append(e0.elapsed_time(e1))
    return float(np.median(ms))


def make_jobs():
    """1024 jobs: sides 180 ... 220, the prior anywhere in the frame, the anchors on two other frames"""
    rng = np.random.default_rng(0)

    def box(f):
        h, w = int(rng.integers(180, 221)), int(rng.integers(180, 221))
        top, left = int(rng.integers(0, H - h + 1)), int(rng.integers(0, W - w + 1))
        return (f, top, left + w, top + h, left)
    jobs = []
    for i in range(N):
        fa = int(rng.integers(0, NF - 4))
        k = int(rng.integers(1, 4))
        jobs.append((*box(fa + k), *box(fa), 4 - k, *box(fa + 4), k))
    return jobs


def build_model():
    cfg = load_config()
    ed = GenConViTED(cfg, init="empty")
    ed.load_state_dict(synth.make_state_dict(spec.ed_spec(), synth.DEFAULT_SEED, "ed/", device="cuda"))
    vae = GenConViTVAE(cfg, init="empty")
    vae.load_state_dict(synth.make_state_dict(spec.vae_spec(include_unused=False), synth.DEFAULT_SEED, "vae/", device="cuda"),
                        strict=False)
    half = lambda m: m.to("cuda").to(torch.float16).eval().reserve(GROUP)
    return GenConViT.from_modules(half(ed), half(vae), net="genconvit")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--out", default="profiles/follow_timing.json")
    a = ap.parse_args()
    torch.set_grad_enabled(False)
    lib = _lib.load()
    frames = torch.randint(0, 256, (NF, H, W, 3), dtype=torch.uint8, generator=torch.Generator().manual_seed(0)).cuda()
    jobs = make_jobs()
    _lib._check_track_jobs("follow_timing", jobs, NF, H, W, GRID)
    jd = torch.tensor(jobs, dtype=torch.int32).cuda()
    out = torch.empty((N, 4), dtype=torch.int32, device="cuda")
    stream = _lib.current_stream_ptr(frames.device)
    boxes = [j[:5] for j in jobs]
    model = build_model()
    eps = synth.make_eps(GROUP, name="follow_timing").cuda()

    def match(radius):
        _lib.check(lib.gcv_track_match(frames.data_ptr(), NF, H, W, jd.data_ptr(), N, GRID, radius, out.data_ptr(), stream),
                   "gcv_track_match")

    def score():
        for g in range(0, N, GROUP):
            model(_lib.face_crop_preprocess(frames, boxes[g:g + GROUP], dtype=torch.float16), eps=eps)
    calls = {"match": lambda: match(RADIUS), "match_r0": lambda: match(0), "score": score}
    res = {"shape": {"frames": [NF, H, W], "jobs": N, "grid": GRID, "radius": RADIUS, "face_sides": [180, 220],
                     "score_group": GROUP}, "steps": a.steps, "rounds": a.rounds, "ms": {k: [] for k in calls}}
    for _ in range(a.rounds):
        for k, call in calls.items():
            res["ms"][k].append(round(median_ms(call, a.steps), 4))
    res["median_ms"] = {k: sorted(v)[len(v) // 2] for k, v in res["ms"].items()}
    res["match_over_score"] = round(res["median_ms"]["match"] / res["median_ms"]["score"], 4)
    match(RADIUS)
    res["jobs_that_moved"] = int((out[:, :2] != 0).any(1).sum())
    print(json.dumps(res))
    os.makedirs(os.path.dirname(a.out) or ".", exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
