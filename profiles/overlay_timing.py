"""Cost of gcv_cam_overlay (csrc/overlay.hip) on one MI355X against its floor and against the same result composed from
torch ops, alternating rounds on one box.  Two shapes:
  (a) clip   15 frames of 1080 x 1920, 15 boxes of about 400 x 400, 7 x 7 maps
  (b) crops  128 crops of 224 x 224, one whole-frame box each, 14 x 14 maps
each timed five ways:
  overlay  _lib.cam_overlay into a preallocated ``out`` (the entry as callers use it: argument checks and the upload of the
           boxes included)
  kernel   gcv_cam_overlay itself through the C ABI, boxes already on the device
  kernel_no_boxes  the same launch with n = 0: the kernel's copy arm alone
  copy     ``out.copy_(frames)``: the floor, the same one read and one write of the frames
  torch    clone, then per box F.interpolate of the map, LUT gather and blend, all on the device (fp32 blend weights as in
           the kernel, integer blend; checked here to give the kernel's pixels)

    python profiles/overlay_timing.py [--steps 50] [--rounds 5] [--out profiles/overlay_timing.json]

Random frames and maps; prints one JSON object and writes it to --out.  GB/s counts one read and one write of the frames
tensor for every variant."""
from __future__ import annotations

import argparse
import json
import os
import sys

import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from genconvit_amd import _lib                                               # noqa: E402


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


def torch_overlay(frames, boxes, maps, lut, alpha=0.5):
    """The weighted overlay from torch ops on the device: one F.interpolate, gather and blend per box."""
    out = frames.clone()
    lut = lut.to(torch.int32)
    for b, (f, top, right, bottom, left) in enumerate(boxes):
        v = F.interpolate(maps[b][None, None], size=(bottom - top, right - left), mode="bilinear",
                          align_corners=False)[0, 0].clamp(0.0, 1.0)
        col = lut[torch.round(v * 255.0).to(torch.int64)]
        a8 = torch.round((alpha * 256.0) * v).to(torch.int32).clamp(0, 256)[..., None]
        region = out[f, top:bottom, left:right]
        region.copy_(((region.to(torch.int32) * (256 - a8) + col * a8 + 128) >> 8).to(torch.uint8))
    return out


def shapes():
    g = torch.Generator().manual_seed(0)
    clip = torch.randint(0, 256, (15, 1080, 1920, 3), dtype=torch.uint8, generator=g)
    clip_boxes = [(f, 200 + 20 * f, 600 + 50 * f + 396 + f, 200 + 20 * f + 404 - f, 600 + 50 * f) for f in range(15)]
    crops = torch.randint(0, 256, (128, 224, 224, 3), dtype=torch.uint8, generator=g)
    crop_boxes = [(i, 0, 224, 224, 0) for i in range(128)]
    return {"clip_15x1080x1920_15boxes_7x7": (clip.cuda(), clip_boxes, torch.rand((15, 7, 7), generator=g).cuda()),
            "crops_128x224x224_14x14": (crops.cuda(), crop_boxes, torch.rand((128, 14, 14), generator=g).cuda())}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--out", default="profiles/overlay_timing.json")
    a = ap.parse_args()
    torch.set_grad_enabled(False)
    lib, lut = _lib.load(), _lib.jet_lut("cuda")
    res = {"steps": a.steps, "rounds": a.rounds, "shapes": {}}
    data = shapes()
    outs = {k: torch.empty_like(v[0]) for k, v in data.items()}
    for name, (frames, boxes, maps) in data.items():
        differs = (_lib.cam_overlay(frames, boxes, maps) != torch_overlay(frames, boxes, maps, lut)).any(-1)
        res["shapes"][name] = {"frame_bytes": frames.numel(), "pixels_torch_composition_differs": int(differs.sum()),
                               "ms": {"overlay": [], "kernel": [], "kernel_no_boxes": [], "copy": [], "torch": []}}
    for _ in range(a.rounds):                 # alternating shapes and variants
        for name, (frames, boxes, maps) in data.items():
            out = outs[name]
            bd = torch.tensor(boxes, dtype=torch.int32).cuda()
            nf, h, w, _ = frames.shape
            stream = _lib.current_stream_ptr(frames.device)
            calls = {"overlay": lambda: _lib.cam_overlay(frames, boxes, maps, out=out),
                     "kernel": lambda: _lib.check(lib.gcv_cam_overlay(
                         frames.data_ptr(), nf, h, w, bd.data_ptr(), len(boxes), maps.data_ptr(), maps.shape[1],
                         maps.shape[2], lut.data_ptr(), 0.5, 1, out.data_ptr(), stream), "gcv_cam_overlay"),
                     "kernel_no_boxes": lambda: _lib.check(lib.gcv_cam_overlay(
                         frames.data_ptr(), nf, h, w, None, 0, None, 0, 0, lut.data_ptr(), 0.5, 1, out.data_ptr(), stream),
                         "gcv_cam_overlay"),
                     "copy": lambda: out.copy_(frames),
                     "torch": lambda: torch_overlay(frames, boxes, maps, lut)}
            for k, call in calls.items():
                res["shapes"][name]["ms"][k].append(round(time_call(call, a.steps), 4))
    for r in res["shapes"].values():
        moved = 2 * r["frame_bytes"]
        r["median_ms"] = {k: sorted(v)[len(v) // 2] for k, v in r["ms"].items()}
        r["gb_per_s"] = {k: round(moved / (r["median_ms"][k] * 1e-3) / 1e9, 1) for k in ("overlay", "kernel", "kernel_no_boxes", "copy")}
        r["kernel_over_copy"] = round(r["median_ms"]["kernel"] / r["median_ms"]["copy"], 3)
        r["overlay_no_slower_than_torch_in_every_round"] = all(o <= t for o, t in zip(r["ms"]["overlay"], r["ms"]["torch"]))
    print(json.dumps(res))
    os.makedirs(os.path.dirname(a.out) or ".", exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
