"""Cost of gcv_face_quality (csrc/quality.hip) on one MI355X beside the upload and the scoring around it.  One shape, the
one a scan with ``quality=True`` meets on 720p footage: 1024 boxes on 8 frames of 720 x 1280, faces of about 200 pixels.
Timed with HIP events, one pair per call, median over --steps calls after warm-up, in alternating rounds:
  quality_g16, quality_g32, quality_g64
               one gcv_face_quality launch through the C ABI at that grid, boxes already on the device
  upload       the 8 frames from pageable host memory to the device (``tensor.to``), what the quality pass of a scan of
               host frames pays a second time
  score        the same 1024 boxes through _lib.face_crop_preprocess and the fp16 ensemble forward (synthetic weights), in
               groups of 128 as scan_frames runs them

    python profiles/quality_timing.py [--steps 20] [--rounds 3] [--out profiles/quality_timing.json]

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

NF, H, W, N, GRIDS, GROUP = 8, 720, 1280, 1024, (16, 32, 64), 128


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


def make_boxes():
    """1024 boxes: sides 180 ... 220, anywhere in any of the frames"""
    rng = np.random.default_rng(0)
    boxes = []
    for _ in range(N):
        h, w = int(rng.integers(180, 221)), int(rng.integers(180, 221))
        top, left = int(rng.integers(0, H - h + 1)), int(rng.integers(0, W - w + 1))
        boxes.append((int(rng.integers(0, NF)), top, left + w, top + h, left))
    return boxes


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
    ap.add_argument("--out", default="profiles/quality_timing.json")
    a = ap.parse_args()
    torch.set_grad_enabled(False)
    lib = _lib.load()
    host = torch.randint(0, 256, (NF, H, W, 3), dtype=torch.uint8, generator=torch.Generator().manual_seed(0))
    frames = host.cuda()
    boxes = make_boxes()
    _lib._check_quality_boxes("quality_timing", boxes, NF, H, W, max(GRIDS))
    bd = torch.tensor(boxes, dtype=torch.int32).cuda()
    out = torch.empty((N, 8), dtype=torch.int64, device="cuda")
    stream = _lib.current_stream_ptr(frames.device)
    model = build_model()
    eps = synth.make_eps(GROUP, name="quality_timing").cuda()

    def measure(grid):
        _lib.check(lib.gcv_face_quality(frames.data_ptr(), NF, H, W, bd.data_ptr(), N, grid, out.data_ptr(), stream),
                   "gcv_face_quality")

    def score():
        for g in range(0, N, GROUP):
            model(_lib.face_crop_preprocess(frames, boxes[g:g + GROUP], dtype=torch.float16), eps=eps)
    calls = {f"quality_g{g}": (lambda g=g: measure(g)) for g in GRIDS}
    calls.update(upload=lambda: host.to("cuda"), score=score)
    res = {"shape": {"frames": [NF, H, W], "boxes": N, "grids": list(GRIDS), "face_sides": [180, 220], "score_group": GROUP},
           "steps": a.steps, "rounds": a.rounds, "ms": {k: [] for k in calls}}
    for _ in range(a.rounds):
        for k, call in calls.items():
            res["ms"][k].append(round(median_ms(call, a.steps), 4))
    res["median_ms"] = {k: sorted(v)[len(v) // 2] for k, v in res["ms"].items()}
    res["quality_over_score"] = {k: round(v / res["median_ms"]["score"], 4) for k, v in res["median_ms"].items()
                                 if k.startswith("quality")}
    measure(max(GRIDS))
    res["rows_measured"] = int((out[:, 0] == max(GRIDS)).sum())
    print(json.dumps(res))
    os.makedirs(os.path.dirname(a.out) or ".", exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
