"""Cost of gcv_yuv420_to_rgb / gcv_rgb_to_yuv420 (csrc/yuv.hip) on one MI355X, and what decoder-native frames save a scan.
Everything from one run, timed with HIP events, one pair per call, median over --steps calls after warm-up, in alternating
rounds.  Per shape (128 frames of 720 x 1280 and of 1080 x 1920, nv12 and i420, bt709 limited):
  to_rgb_<layout>   one gcv_yuv420_to_rgb launch through the C ABI on uniform-noise bytes: 1.5 bytes in, 3 out per pixel
  to_yuv_<layout>   one gcv_rgb_to_yuv420 launch: 3 in, 1.5 out
  copy              a device-to-device copy that reads the YUV bytes and one that writes the RGB bytes' worth: 4.5 bytes a
                    pixel moved each way, the same bytes in plus out as either converter
  hist              one gcv_frame_hist launch (regions = 4) on the RGB frames: the streaming kernel the scan already has
  h2d_yuv, h2d_rgb  the host-to-device copy of the YUV and of the RGB form of the frames, from pageable memory as
                    ``scan_frames`` does it; d2h_* the way back
and at 720p, with the fp16 ensemble on synthetic weights and one 200-pixel face box on each of 256 host frames:
  scan_rgb, scan_yuv      ``scan_frames`` from host RGB frames and from the same pixels as a host ``YUV420`` (wall clock
                          around a synchronised call)
  render_rgb, render_nv12 ``render_scan`` of that result, RGB in and out against ``YUV420`` in and out="nv12"

    python profiles/yuv_timing.py [--steps 20] [--rounds 3] [--out profiles/yuv_timing.json]

Prints one JSON object and writes it to --out.  bytes_per_s counts bytes read plus bytes written over the launch time."""
from __future__ import annotations

import argparse
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from genconvit_amd import _lib, spec, synth                                  # noqa: E402
from genconvit_amd.model import pred_func                                    # noqa: E402
from genconvit_amd.model.config import load_config                           # noqa: E402
from genconvit_amd.model.genconvit import GenConViT                          # noqa: E402
from genconvit_amd.model.genconvit_ed import GenConViTED                     # noqa: E402
from genconvit_amd.model.genconvit_vae import GenConViTVAE                   # noqa: E402

NF, SHAPES, SCAN_FRAMES, FACE = 128, ((720, 1280), (1080, 1920)), 256, 200


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


def wall_ms(call, steps, warmup=1):
    for _ in range(warmup):
        call()
    ms = []
    for _ in range(steps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        call()
        torch.cuda.synchronize()
        ms.append((time.perf_counter() - t0) * 1e3)
    return float(np.median(ms))


def build_model(batch):
    cfg = load_config()
    ed = GenConViTED(cfg, init="empty")
    ed.load_state_dict(synth.make_state_dict(spec.ed_spec(), synth.DEFAULT_SEED, "ed/", device="cuda"))
    vae = GenConViTVAE(cfg, init="empty")
    vae.load_state_dict(synth.make_state_dict(spec.vae_spec(include_unused=False), synth.DEFAULT_SEED, "vae/", device="cuda"),
                        strict=False)
    half = lambda m: m.to("cuda").to(torch.float16).eval().reserve(batch)
    return GenConViT.from_modules(half(ed), half(vae), net="genconvit")


def kernels(h, w, steps, rounds):
    lib, stream = _lib.load(), _lib.current_stream_ptr(torch.device("cuda"))
    gen = torch.Generator().manual_seed(h)
    host_yuv = torch.randint(0, 256, (NF, 3 * h // 2, w), dtype=torch.uint8, generator=gen)
    host_rgb = torch.randint(0, 256, (NF, h, w, 3), dtype=torch.uint8, generator=gen)
    yuv, rgb = host_yuv.cuda(), host_rgb.cuda()
    yuv2, rgb2 = torch.empty_like(yuv), torch.empty_like(rgb)
    back_yuv, back_rgb = torch.empty_like(host_yuv), torch.empty_like(host_rgb)
    hist = torch.empty((NF, 16, _lib.CUT_BINS), dtype=torch.int32, device="cuda")

    def to_rgb(layout):
        _lib.check(lib.gcv_yuv420_to_rgb(yuv.data_ptr(), NF, h, w, layout, 1, 0, rgb2.data_ptr(), stream), "gcv_yuv420_to_rgb")

    def to_yuv(layout):
        _lib.check(lib.gcv_rgb_to_yuv420(rgb.data_ptr(), NF, h, w, layout, 1, 0, yuv2.data_ptr(), stream), "gcv_rgb_to_yuv420")

    def copy():                                             # reads 1.5 + 3 and writes 1.5 + 3 bytes a pixel: halve it below
        yuv2.copy_(yuv)
        rgb2.copy_(rgb)
    calls = {
        "to_rgb_i420": lambda: to_rgb(0), "to_rgb_nv12": lambda: to_rgb(1),
        "to_yuv_i420": lambda: to_yuv(0), "to_yuv_nv12": lambda: to_yuv(1),
        "copy_both": copy,
        "hist": lambda: _lib.check(lib.gcv_frame_hist(rgb.data_ptr(), NF, h, w, 4, hist.data_ptr(), stream), "gcv_frame_hist"),
        "h2d_yuv": lambda: yuv2.copy_(host_yuv), "h2d_rgb": lambda: rgb2.copy_(host_rgb),
        "d2h_yuv": lambda: back_yuv.copy_(yuv), "d2h_rgb": lambda: back_rgb.copy_(rgb),
    }
    ms = {k: [] for k in calls}
    for _ in range(rounds):
        for k, call in calls.items():
            ms[k].append(round(median_ms(call, steps), 4))
    med = {k: sorted(v)[len(v) // 2] for k, v in ms.items()}
    med["copy"] = round(med["copy_both"] / 2, 4)            # the bytes of one converter: 4.5 a pixel in plus out
    moved = NF * h * w * 9 // 2
    out = {"frames": [NF, h, w], "ms": ms, "median_ms": med, "bytes_in_plus_out": moved,
           "bytes_per_s": {k: round(moved / (med[k] * 1e-3)) for k in ("to_rgb_i420", "to_rgb_nv12", "to_yuv_i420", "to_yuv_nv12",
                                                                       "copy")},
           "hist_bytes_per_s": round(NF * h * w * 3 / (med["hist"] * 1e-3))}
    out["rate_over_copy"] = {k: round(med["copy"] / med[k], 4) for k in ("to_rgb_i420", "to_rgb_nv12", "to_yuv_i420", "to_yuv_nv12")}
    # what was timed is what the tests check: a converted frame against the binding's own result on a slice
    to_rgb(1)
    assert torch.equal(rgb2[:2], _lib.yuv420_to_rgb(yuv[:2], "nv12"))
    to_yuv(0)
    assert torch.equal(yuv2[-2:], _lib.rgb_to_yuv420(rgb[-2:], "i420"))
    return out


def end_to_end(steps):
    h, w = SHAPES[0]
    gen = torch.Generator().manual_seed(9)
    yuv = torch.randint(0, 256, (SCAN_FRAMES, 3 * h // 2, w), dtype=torch.uint8, generator=gen)
    frames = pred_func.YUV420(yuv, "nv12")
    rgb = torch.cat([frames.rgb(slice(g, g + 64)).cpu() for g in range(0, SCAN_FRAMES, 64)]).numpy()
    rng = np.random.default_rng(0)
    boxes = []
    for f in range(SCAN_FRAMES):
        top, left = int(rng.integers(0, h - FACE + 1)), int(rng.integers(0, w - FACE + 1))
        boxes.append((f, top, left + FACE, top + FACE, left))
    model = build_model(128)
    eps = synth.make_eps(SCAN_FRAMES, name="yuv_timing").cuda()
    kw = dict(boxes=boxes, eps=eps, iou=2.0)                # iou 2: every box its own track, the rows stay in frame order
    res = pred_func.scan_frames(rgb, model, **kw)
    res_yuv = pred_func.scan_frames(frames, model, **kw)
    assert torch.equal(res["frame_scores"], res_yuv["frame_scores"]) and len(res["boxes"]) == SCAN_FRAMES
    calls = {
        "scan_rgb": lambda: pred_func.scan_frames(rgb, model, **kw),
        "scan_yuv": lambda: pred_func.scan_frames(frames, model, **kw),
        "render_rgb": lambda: pred_func.render_scan(rgb, res, model, eps=eps),
        "render_nv12": lambda: pred_func.render_scan(frames, res, model, eps=eps, out="nv12"),
    }
    ms = {k: round(wall_ms(call, steps), 3) for k, call in calls.items()}
    return {"frames": [SCAN_FRAMES, h, w], "face_side": FACE, "steps": steps, "wall_ms": ms,
            "scan_yuv_over_rgb": round(ms["scan_yuv"] / ms["scan_rgb"], 4),
            "render_nv12_over_rgb": round(ms["render_nv12"] / ms["render_rgb"], 4)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--scan-steps", type=int, default=5)
    ap.add_argument("--out", default="profiles/yuv_timing.json")
    a = ap.parse_args()
    torch.set_grad_enabled(False)
    res = {"steps": a.steps, "rounds": a.rounds, "kernels": {f"{h}x{w}": kernels(h, w, a.steps, a.rounds) for h, w in SHAPES},
           "end_to_end": end_to_end(a.scan_steps)}
    print(json.dumps(res))
    os.makedirs(os.path.dirname(a.out) or ".", exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
