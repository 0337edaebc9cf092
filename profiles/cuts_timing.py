"""Cost of gcv_frame_hist / gcv_hist_diff (csrc/cuts.hip) on one MI355X beside what a scan already does with the same
frames.  One shape, a group of a whole-video scan on 720p footage: 128 frames of 720 x 1280, regions = 4.  Timed with HIP
events, one pair per call, median over --steps calls after warm-up, in alternating rounds:
  hist          one gcv_frame_hist launch through the C ABI on uniform-noise frames (every bin of every region is hit)
  hist_smooth   the same launch on smooth frames (a colour ramp with +-6 noise: neighbouring pixels share a bin, the case
                the 32 LDS columns per bin are for)
  hist_r1       regions = 1 on the noise frames: 128 regions, each split over 8 workgroups merged by atomic adds, behind
                the memset of the output
  diff          one gcv_hist_diff launch over the 128 histograms at regions = 4
  upload        the host-to-device copy of the 128 frames from pinned memory
  upload_paged  the same copy from pageable memory, as ``scan_frames`` does it
  score         _lib.face_crop_preprocess plus the fp16 ensemble forward (synthetic weights) of one 200-pixel face per
                frame, one group of 128: the work a scan already does on these frames

    python profiles/cuts_timing.py [--steps 20] [--rounds 3] [--out profiles/cuts_timing.json]

Prints one JSON object and writes it to --out.  bytes_per_s is the frames' bytes, read once, over the launch time."""
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

NF, H, W, REGIONS, FACE = 128, 720, 1280, 4, 200


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


def smooth_frames(gen):
    """a horizontal and a vertical colour ramp with +-6 noise per channel"""
    y = torch.arange(H).view(1, H, 1, 1)
    x = torch.arange(W).view(1, 1, W, 1)
    base = torch.cat((40 + 120 * x // W + 0 * y, 60 + 90 * y // H + 0 * x, 90 + 40 * x // W + 30 * y // H), 3)
    return (base.to(torch.int16) + torch.randint(-6, 7, (NF, H, W, 3), generator=gen, dtype=torch.int16)).clamp_(0, 255).to(torch.uint8)


def build_model():
    cfg = load_config()
    ed = GenConViTED(cfg, init="empty")
    ed.load_state_dict(synth.make_state_dict(spec.ed_spec(), synth.DEFAULT_SEED, "ed/", device="cuda"))
    vae = GenConViTVAE(cfg, init="empty")
    vae.load_state_dict(synth.make_state_dict(spec.vae_spec(include_unused=False), synth.DEFAULT_SEED, "vae/", device="cuda"),
                        strict=False)
    half = lambda m: m.to("cuda").to(torch.float16).eval().reserve(NF)
    return GenConViT.from_modules(half(ed), half(vae), net="genconvit")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--out", default="profiles/cuts_timing.json")
    a = ap.parse_args()
    torch.set_grad_enabled(False)
    lib = _lib.load()
    gen = torch.Generator().manual_seed(0)
    host = torch.randint(0, 256, (NF, H, W, 3), dtype=torch.uint8, generator=gen)
    pinned = host.pin_memory()
    noise, smooth = host.cuda(), smooth_frames(gen).cuda()
    landing = torch.empty_like(noise)
    stream = _lib.current_stream_ptr(noise.device)
    hist = torch.empty((NF, REGIONS * REGIONS, _lib.CUT_BINS), dtype=torch.int32, device="cuda")
    hist1 = torch.empty((NF, 1, _lib.CUT_BINS), dtype=torch.int32, device="cuda")
    dist = torch.empty((NF - 1, REGIONS * REGIONS), dtype=torch.int32, device="cuda")
    rng = np.random.default_rng(0)
    boxes = []
    for f in range(NF):
        top, left = int(rng.integers(0, H - FACE + 1)), int(rng.integers(0, W - FACE + 1))
        boxes.append((f, top, left + FACE, top + FACE, left))
    model = build_model()
    eps = synth.make_eps(NF, name="cuts_timing").cuda()

    def frame_hist(frames, regions, out):
        _lib.check(lib.gcv_frame_hist(frames.data_ptr(), NF, H, W, regions, out.data_ptr(), stream), "gcv_frame_hist")

    def score():
        model(_lib.face_crop_preprocess(noise, boxes, dtype=torch.float16), eps=eps)
    calls = {
        "hist": lambda: frame_hist(noise, REGIONS, hist),
        "hist_smooth": lambda: frame_hist(smooth, REGIONS, hist),
        "hist_r1": lambda: frame_hist(noise, 1, hist1),
        "diff": lambda: _lib.check(lib.gcv_hist_diff(hist.data_ptr(), NF, REGIONS, dist.data_ptr(), stream), "gcv_hist_diff"),
        "upload": lambda: landing.copy_(pinned, non_blocking=True),
        "upload_paged": lambda: landing.copy_(host),
        "score": score,
    }
    res = {"shape": {"frames": [NF, H, W], "regions": REGIONS, "face_side": FACE, "score_group": NF}, "steps": a.steps,
           "rounds": a.rounds, "ms": {k: [] for k in calls}}
    for _ in range(a.rounds):
        for k, call in calls.items():
            res["ms"][k].append(round(median_ms(call, a.steps), 4))
    res["median_ms"] = {k: sorted(v)[len(v) // 2] for k, v in res["ms"].items()}
    nbytes = NF * H * W * 3
    res["frame_bytes"] = nbytes
    res["bytes_per_s"] = {k: round(nbytes / (res["median_ms"][k] * 1e-3)) for k in ("hist", "hist_smooth", "hist_r1", "upload",
                                                                                  "upload_paged")}
    res["hist_over_score"] = round(res["median_ms"]["hist"] / res["median_ms"]["score"], 4)
    res["hist_over_upload"] = round(res["median_ms"]["hist"] / res["median_ms"]["upload"], 4)
    # what was timed is what the tests check: the three histograms add up to the pixels
    frame_hist(noise, REGIONS, hist)
    frame_hist(noise, 1, hist1)
    assert int(hist.sum()) == int(hist1.sum()) == NF * H * W and torch.equal(hist.sum(1), hist1[:, 0].long())
    print(json.dumps(res))
    os.makedirs(os.path.dirname(a.out) or ".", exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
