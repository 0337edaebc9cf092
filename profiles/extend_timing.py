"""Cost of gcv_track_chain (csrc/follow.hip) on one MI355X beside the scoring it feeds.  One shape, the one a scan with
``extend=True`` meets on 720p footage: 32 chains of 32 steps on 33 frames of 720 x 1280, faces of about 200 pixels, grid
64, radius 8 — 1024 boxes in all.  Timed with HIP events, one pair per call, median over --steps calls after warm-up, in
alternating rounds:
  chain        one gcv_track_chain launch through the C ABI, jobs already on the device
  chain_1      the same 32 chains cut to one step: the launch, the template and one step
  chain_r0     32 steps at radius 0: the window without its margin and one candidate per step
  score        1024 boxes of those sizes through _lib.face_crop_preprocess and the fp16 ensemble forward (synthetic
               weights), in groups of 128 as scan_frames runs them (--no-score leaves it out)
A launch of 32 workgroups on 256 CUs is bound by steps x the latency of one step, so (chain - chain_1) / 31 is printed
as the time of a step.

    python profiles/extend_timing.py [--steps 20] [--rounds 3] [--label TEXT] [--out profiles/extend_timing.json]

Random frames; prints one JSON object and writes it to --out.  --label is copied into the record (the workgroup-size A/B
of profiles/extend_threads_ab.json runs this script once per build)."""
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

CHAINS, STEPS, H, W, GRID, RADIUS, GROUP = 32, 32, 720, 1280, 64, 8, 128
NF = STEPS + 1
STOP_NEVER = 2 ** 31 - 1


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


def make_jobs(steps):
    """32 chains: sides 180 ... 220, the template anywhere in frame 0 (forward) or the last frame (backward)"""
    rng = np.random.default_rng(0)
    jobs = []
    for i in range(CHAINS):
        h, w = int(rng.integers(180, 221)), int(rng.integers(180, 221))
        top, left = int(rng.integers(0, H - h + 1)), int(rng.integers(0, W - w + 1))
        fa, fs, d = (0, 1, 1) if i % 2 == 0 else (NF - 1, NF - 2, -1)
        jobs.append((fa, top, left + w, top + h, left, fs, d, steps, 0, 0, STOP_NEVER))
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
    ap.add_argument("--label", default="")
    ap.add_argument("--no-score", action="store_true")
    ap.add_argument("--out", default="profiles/extend_timing.json")
    a = ap.parse_args()
    torch.set_grad_enabled(False)
    lib = _lib.load()
    frames = torch.randint(0, 256, (NF, H, W, 3), dtype=torch.uint8, generator=torch.Generator().manual_seed(0)).cuda()
    jobs, jobs1 = make_jobs(STEPS), make_jobs(1)
    for j in (jobs, jobs1):
        _lib._check_chain_jobs("extend_timing", j, NF, H, W, GRID)
    jd, jd1 = torch.tensor(jobs, dtype=torch.int32).cuda(), torch.tensor(jobs1, dtype=torch.int32).cuda()
    out = torch.empty((CHAINS, STEPS, 4), dtype=torch.int32, device="cuda")
    stream = _lib.current_stream_ptr(frames.device)

    def chain(rows, steps, radius):
        _lib.check(lib.gcv_track_chain(frames.data_ptr(), NF, H, W, rows.data_ptr(), CHAINS, steps, GRID, radius,
                                       out.data_ptr(), stream), "gcv_track_chain")
    calls = {"chain": lambda: chain(jd, STEPS, RADIUS), "chain_1": lambda: chain(jd1, 1, RADIUS),
             "chain_r0": lambda: chain(jd, STEPS, 0)}
    if not a.no_score:
        boxes = [(k % NF, *j[1:5]) for j in jobs for k in range(STEPS)]
        model = build_model()
        eps = synth.make_eps(GROUP, name="extend_timing").cuda()

        def score():
            for g in range(0, len(boxes), GROUP):
                model(_lib.face_crop_preprocess(frames, boxes[g:g + GROUP], dtype=torch.float16), eps=eps)
        calls["score"] = score
    res = {"shape": {"frames": [NF, H, W], "chains": CHAINS, "chain_steps": STEPS, "grid": GRID, "radius": RADIUS,
                     "face_sides": [180, 220], "score_group": GROUP}, "label": a.label, "steps": a.steps, "rounds": a.rounds,
           "ms": {k: [] for k in calls}}
    for _ in range(a.rounds):
        for k, call in calls.items():
            res["ms"][k].append(round(median_ms(call, a.steps), 4))
    res["median_ms"] = {k: sorted(v)[len(v) // 2] for k, v in res["ms"].items()}
    res["ms_per_step"] = round((res["median_ms"]["chain"] - res["median_ms"]["chain_1"]) / (STEPS - 1), 5)
    if "score" in calls:
        res["chain_over_score"] = round(res["median_ms"]["chain"] / res["median_ms"]["score"], 4)
    chain(jd, STEPS, RADIUS)
    got = out.cpu()
    res["steps_that_moved"] = int((got[:, :, :2] != 0).any(2).sum())
    res["checksum"] = int(got.long().sum())
    print(json.dumps(res))
    os.makedirs(os.path.dirname(a.out) or ".", exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
