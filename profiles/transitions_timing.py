"""Cost of gcv_frame_cells / gcv_blend_fit / gcv_hist_diff_lag (csrc/cuts.hip) on one MI355X beside what a scan already
does with the same frames.  One shape, a group of a whole-video scan on 720p footage: 128 frames of 720 x 1280.  Timed
with HIP events, one pair per call, median over --steps calls after warm-up, in alternating rounds:
  cells_g8, cells_g16, cells_g32    one gcv_frame_cells launch through the C ABI on uniform-noise frames at each grid
  cells_g16_smooth                  the same launch at G = 16 on smooth frames (a colour ramp with +-6 noise)
  hist                              one gcv_frame_hist launch at regions = 4 on the noise frames: it reads the same bytes
  fit_l4, fit_l8                    one gcv_blend_fit launch over the 128 rows of cells at G = 16
  fit_g32_l8                        the same at G = 32, four cells a thread
  diff_l4, diff_l8                  one gcv_hist_diff_lag launch over the 128 histograms at regions = 4
  upload                            the host-to-device copy of the 128 frames from pinned memory
  upload_paged                      the same copy from pageable memory, as ``scan_frames`` does it
  score                             _lib.face_crop_preprocess plus the fp16 ensemble forward (synthetic weights) of one
                                    200-pixel face per frame, one group of 128: the work a scan already does on these frames

    python profiles/transitions_timing.py [--steps 20] [--rounds 3] [--out profiles/transitions_timing.json]

Prints one JSON object and writes it to --out.  bytes_per_s is the frames' bytes, read once, over the launch time."""
from __future__ import annotations

import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from cuts_timing import FACE, H, NF, W, build_model, median_ms, smooth_frames     # noqa: E402
from genconvit_amd import _lib, synth                                             # noqa: E402

REGIONS, GRIDS, LAGS = 4, (8, 16, 32), (4, 8)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--out", default="profiles/transitions_timing.json")
    a = ap.parse_args()
    torch.set_grad_enabled(False)
    lib = _lib.load()
    gen = torch.Generator().manual_seed(0)
    host = torch.randint(0, 256, (NF, H, W, 3), dtype=torch.uint8, generator=gen)
    pinned = host.pin_memory()
    noise, smooth = host.cuda(), smooth_frames(gen).cuda()
    landing = torch.empty_like(noise)
    stream = _lib.current_stream_ptr(noise.device)
    cells = {g: torch.empty((NF, g * g), dtype=torch.int32, device="cuda") for g in GRIDS}
    hist = torch.empty((NF, REGIONS * REGIONS, _lib.CUT_BINS), dtype=torch.int32, device="cuda")
    fit = torch.empty((NF, 2 * max(LAGS) - 1), dtype=torch.int64, device="cuda")
    dist = torch.empty((NF, REGIONS * REGIONS), dtype=torch.int32, device="cuda")
    rng = np.random.default_rng(0)
    boxes = []
    for f in range(NF):
        top, left = int(rng.integers(0, H - FACE + 1)), int(rng.integers(0, W - FACE + 1))
        boxes.append((f, top, left + FACE, top + FACE, left))
    model = build_model()
    eps = synth.make_eps(NF, name="cuts_timing").cuda()

    def frame_cells(frames, grid):
        _lib.check(lib.gcv_frame_cells(frames.data_ptr(), NF, H, W, grid, cells[grid].data_ptr(), stream), "gcv_frame_cells")

    def blend_fit(grid, lag):
        _lib.check(lib.gcv_blend_fit(cells[grid].data_ptr(), NF, grid, lag, fit.data_ptr(), stream), "gcv_blend_fit")

    def hist_diff_lag(lag):
        _lib.check(lib.gcv_hist_diff_lag(hist.data_ptr(), NF, REGIONS, lag, dist.data_ptr(), stream), "gcv_hist_diff_lag")

    def score():
        model(_lib.face_crop_preprocess(noise, boxes, dtype=torch.float16), eps=eps)
    calls = {f"cells_g{g}": (lambda g=g: frame_cells(noise, g)) for g in GRIDS}
    calls["cells_g16_smooth"] = lambda: frame_cells(smooth, 16)
    calls["hist"] = lambda: _lib.check(lib.gcv_frame_hist(noise.data_ptr(), NF, H, W, REGIONS, hist.data_ptr(), stream),
                                       "gcv_frame_hist")
    calls.update({f"fit_l{lag}": (lambda lag=lag: blend_fit(16, lag)) for lag in LAGS})
    calls["fit_g32_l8"] = lambda: blend_fit(32, 8)
    calls.update({f"diff_l{lag}": (lambda lag=lag: hist_diff_lag(lag)) for lag in LAGS})
    calls.update({"upload": lambda: landing.copy_(pinned, non_blocking=True), "upload_paged": lambda: landing.copy_(host),
                  "score": score})
    for g in GRIDS:                                         # the fits and the distances read what these leave
        frame_cells(noise, g)
    calls["hist"]()
    res = {"shape": {"frames": [NF, H, W], "grids": list(GRIDS), "fit_grid": 16, "lags": list(LAGS), "regions": REGIONS,
                     "face_side": FACE, "score_group": NF}, "steps": a.steps, "rounds": a.rounds, "ms": {k: [] for k in calls}}
    for _ in range(a.rounds):
        for k, call in calls.items():
            res["ms"][k].append(round(median_ms(call, a.steps), 4))
    res["median_ms"] = {k: sorted(v)[len(v) // 2] for k, v in res["ms"].items()}
    nbytes = NF * H * W * 3
    res["frame_bytes"] = nbytes
    res["bytes_per_s"] = {k: round(nbytes / (res["median_ms"][k] * 1e-3)) for k in res["median_ms"]
                          if k.startswith(("cells", "hist", "upload"))}
    res["cells_g16_over_hist"] = round(res["median_ms"]["cells_g16"] / res["median_ms"]["hist"], 4)
    res["cells_g16_over_score"] = round(res["median_ms"]["cells_g16"] / res["median_ms"]["score"], 4)
    res["cells_g16_over_upload"] = round(res["median_ms"]["cells_g16"] / res["median_ms"]["upload"], 4)
    # what was timed is what the tests check: at every grid the cells of a frame add up to the same total luma
    for g in GRIDS:
        frame_cells(noise, g)
    assert torch.equal(cells[8].sum(1), cells[16].sum(1)) and torch.equal(cells[8].sum(1), cells[32].sum(1))
    # and 720 x 1280 divides by 16 both ways, so a cell at G = 8 is exactly four cells at G = 16
    assert torch.equal(cells[16].view(NF, 8, 2, 8, 2).sum((2, 4)), cells[8].view(NF, 8, 8))
    print(json.dumps(res))
    os.makedirs(os.path.dirname(a.out) or ".", exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
