"""Cost of gcv_scan_annotate (csrc/annotate.hip) on one MI355X against its two yardsticks from the same run, alternating
rounds on one box, and the wall time of ``pred_func.render_scan`` beside the ``scan_frames`` whose result it draws.
  (a) the kernel: 128 frames of 720 x 1280, 128 marks (one box of 280 ... 360 pixels a side with a label per frame, thick 3)
      and the default strip of 20 rows over a (2, 128) timeline, through the C ABI with everything on the device, each call
      timed with HIP events:
        annotate_in_place    out == frames: one read, and writes only where something is drawn
        annotate_out         into a second buffer: one read and one write of the frames
        copy                 ``out.copy_(frames)``: the floor of annotate_out, the same bytes
        cam_overlay_out      gcv_cam_overlay with the same 128 boxes and 7 x 7 maps into the second buffer: more arithmetic
        cam_overlay_in_place per covered pixel (a bilinear sample, a LUT gather and a blend)
        binding_in_place     ``_lib.scan_annotate(..., out=frames)``: argument checks and the uploads of the marks included
  (b) the stage: 256 host frames of 720 x 1280, one face a frame, the fp16 ensemble with synthetic weights:
      ``scan_frames`` (boxes given, eps pinned), ``render_scan`` of its result as it is, without evidence, and with a
      segment over frames 64 ... 127 added so that 64 rows get their evidence drawn — host wall time of whole calls, which
      end in the copy of the frames back to the host.

    python profiles/render_timing.py [--steps 50] [--rounds 5] [--out profiles/render_timing.json]

Random frames; prints one JSON object and writes it to --out.  GB/s counts one read and one write of the frames."""
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

NF, H, W, THICK, STRIP = 128, 720, 1280, 3, 20
NF_STAGE = 256


def median_ms(call, steps):
    for _ in range(3):
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


def wall_s(call):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    call()
    torch.cuda.synchronize()
    return time.perf_counter() - t0


def make_boxes(nf):
    """one box a frame, 280 ... 360 pixels a side, drifting up and down and left and right: one track for ``scan_frames``"""
    boxes = []
    for f in range(nf):
        h, w = 280 + (7 * f) % 81, 280 + (11 * f) % 81
        top, left = 100 + abs((3 * f) % 400 - 200), 300 + abs((5 * f) % 1000 - 500)
        boxes.append((f, top, left + w, top + h, left))
    return boxes


def build_model():
    cfg = load_config()
    ed = GenConViTED(cfg, init="empty")
    ed.load_state_dict(synth.make_state_dict(spec.ed_spec(), synth.DEFAULT_SEED, "ed/", device="cuda"))
    vae = GenConViTVAE(cfg, init="empty")
    vae.load_state_dict(synth.make_state_dict(spec.vae_spec(include_unused=False), synth.DEFAULT_SEED, "vae/", device="cuda"),
                        strict=False)
    half = lambda m: m.to("cuda").to(torch.float16).eval()
    return GenConViT.from_modules(half(ed), half(vae), net="genconvit")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--out", default="profiles/render_timing.json")
    a = ap.parse_args()
    torch.set_grad_enabled(False)
    lib = _lib.load()
    g = torch.Generator().manual_seed(0)
    host = torch.randint(0, 256, (NF_STAGE, H, W, 3), dtype=torch.uint8, generator=g)
    frames = host[:NF].cuda()
    out = torch.empty_like(frames)
    boxes = make_boxes(NF_STAGE)
    lut = _lib.jet_lut("cuda")
    colours = (lut.cpu().long()[:, 0] | lut.cpu().long()[:, 1] << 8 | lut.cpu().long()[:, 2] << 16).tolist()
    marks = [(*b, colours[(37 * i) % 256], THICK, i) for i, b in enumerate(boxes[:NF])]
    timeline = torch.randint(0, 1 << 24, (2, NF), dtype=torch.int64, generator=g)
    md = torch.tensor(marks, dtype=torch.int32).cuda()
    bd = torch.tensor(boxes[:NF], dtype=torch.int32).cuda()
    fno = torch.arange(NF, dtype=torch.int32).cuda()
    tl = timeline.to(torch.int32).cuda()
    maps = torch.rand((NF, 7, 7), generator=g).cuda()
    stream = _lib.current_stream_ptr(frames.device)

    def annotate(dst):
        _lib.check(lib.gcv_scan_annotate(frames.data_ptr(), NF, H, W, fno.data_ptr(), md.data_ptr(), NF, tl.data_ptr(), 2, NF,
                                         STRIP, dst.data_ptr(), stream), "gcv_scan_annotate")

    def overlay(dst):
        _lib.check(lib.gcv_cam_overlay(frames.data_ptr(), NF, H, W, bd.data_ptr(), NF, maps.data_ptr(), 7, 7, lut.data_ptr(),
                                       0.5, 1, dst.data_ptr(), stream), "gcv_cam_overlay")
    calls = {"annotate_out": lambda: annotate(out), "copy": lambda: out.copy_(frames), "cam_overlay_out": lambda: overlay(out),
             "annotate_in_place": lambda: annotate(frames), "cam_overlay_in_place": lambda: overlay(frames),
             "binding_in_place": lambda: _lib.scan_annotate(frames, fno, marks, timeline, STRIP, out=frames)}
    covered = sum((b[3] - b[1]) * (b[2] - b[4]) for b in boxes[:NF])
    res = {"shape": {"frames": [NF, H, W], "marks": NF, "box_sides": [280, 360], "thick": THICK, "strip": STRIP,
                     "timeline": [2, NF], "maps": [7, 7], "frame_bytes": frames.numel(),
                     "pixels_inside_boxes": covered, "pixels": NF * H * W},
           "steps": a.steps, "rounds": a.rounds, "ms": {k: [] for k in calls}}
    for _ in range(a.rounds):                 # alternating variants
        for k, call in calls.items():
            res["ms"][k].append(round(median_ms(call, a.steps), 4))
    med = res["median_ms"] = {k: sorted(v)[len(v) // 2] for k, v in res["ms"].items()}
    res["spread_ms"] = {k: round(max(v) - min(v), 4) for k, v in res["ms"].items()}
    res["gb_per_s"] = {k: round(2 * frames.numel() / (med[k] * 1e-3) / 1e9, 1) for k in ("annotate_out", "copy", "cam_overlay_out")}
    res["annotate_out_over_copy"] = round(med["annotate_out"] / med["copy"], 3)
    res["annotate_out_over_cam_overlay_out"] = round(med["annotate_out"] / med["cam_overlay_out"], 3)
    res["annotate_in_place_over_cam_overlay_in_place"] = round(med["annotate_in_place"] / med["cam_overlay_in_place"], 3)

    # (b) the stage beside the scan
    del frames, out
    model = build_model()
    eps = synth.make_eps(NF_STAGE, name="render_timing").cuda()
    small = host[:8].numpy()
    warm = pred_func.scan_frames(small, model, boxes=boxes[:8], eps=eps[:8])
    pred_func.render_scan(small, dict(warm, segments=[(0, 0, 7, 1.0)]), model, eps=eps[:8])
    frames_np = host.numpy()
    stage = {"scan_frames": [], "render_scan": [], "render_scan_no_evidence": [], "render_scan_64_evidence_rows": []}
    for _ in range(3):
        kept = {}
        stage["scan_frames"].append(wall_s(lambda: kept.update(res=pred_func.scan_frames(frames_np, model, boxes=boxes, eps=eps))))
        scan = kept["res"]
        forced = dict(scan, segments=list(scan["segments"]) + [(0, 64, 127, 1.0)])
        stage["render_scan"].append(wall_s(lambda: pred_func.render_scan(frames_np, scan, model, eps=eps)))
        stage["render_scan_no_evidence"].append(wall_s(lambda: pred_func.render_scan(frames_np, scan, model, evidence=False)))
        stage["render_scan_64_evidence_rows"].append(wall_s(lambda: pred_func.render_scan(frames_np, forced, model, eps=eps)))
    rows = scan["boxes"]
    res["stage"] = {"frames": [NF_STAGE, H, W], "crops": len(rows), "tracks": len(scan["tracks"]),
                    "segments_of_the_scan": len(scan["segments"]),
                    "evidence_rows_of_the_scan": len({i for t, first, last, _ in scan["segments"]
                                                      for i in range(scan["track_offsets"][t], scan["track_offsets"][t + 1])
                                                      if first <= rows[i][0] <= last}),
                    "wall_s": {k: [round(x, 4) for x in v] for k, v in stage.items()},
                    "median_wall_s": {k: round(sorted(v)[1], 4) for k, v in stage.items()}}
    m = res["stage"]["median_wall_s"]
    res["stage"]["render_no_evidence_over_scan"] = round(m["render_scan_no_evidence"] / m["scan_frames"], 3)
    res["stage"]["render_64_evidence_rows_over_scan"] = round(m["render_scan_64_evidence_rows"] / m["scan_frames"], 3)
    print(json.dumps(res))
    os.makedirs(os.path.dirname(a.out) or ".", exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
