"""Cost of gcv_face_signature and gcv_sig_link (csrc/persons.hip) on one MI355X beside the scoring of the same faces and
the numpy restatement of the link.  The shapes a scan with ``persons=True`` meets on 720p footage: 1024 boxes of about
200 pixels on 8 frames of 720 x 1280; 4096 signatures of 64 tracks for the link.
Timed with HIP events, one pair per call, median over --steps calls after warm-up, in alternating rounds:
  signature      one gcv_face_signature launch through the C ABI, boxes already on the device
  link           one gcv_sig_link call through the C ABI (its memset and its launch) at n = 4096, T = 64, the rows of a
                 track contiguous, as scan_frames hands them over
  link_shuffled  the same rows in random order: no two neighbouring pairs share their tracks, so hardly any minimum is
                 merged before the atomics
  score          the same 1024 boxes through _lib.face_crop_preprocess and the fp16 ensemble forward (synthetic weights), in
                 groups of 128 as scan_frames runs them
and, with the wall clock, once: ``link_numpy_s``, tests/personutil.sig_link_ref on the same 4096 rows on the host, whose
result the device's must equal (``link_equals_restatement``).

    python profiles/persons_timing.py [--steps 20] [--rounds 3] [--out profiles/persons_timing.json]

Random frames and random signature bytes; prints one JSON object and writes it to --out."""
from __future__ import annotations

import argparse
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from genconvit_amd import _lib, synth                                        # noqa: E402
from quality_timing import GROUP, H, N, NF, W, build_model, make_boxes, median_ms   # noqa: E402
from tests import personutil as pu                                           # noqa: E402

ROWS, TRACKS = 4096, 64


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--out", default="profiles/persons_timing.json")
    a = ap.parse_args()
    torch.set_grad_enabled(False)
    lib = _lib.load()
    host = torch.randint(0, 256, (NF, H, W, 3), dtype=torch.uint8, generator=torch.Generator().manual_seed(0))
    frames = host.cuda()
    boxes = make_boxes()
    _lib._check_quality_boxes("persons_timing", boxes, NF, H, W, _lib.SIG_GRID)
    bd = torch.tensor(boxes, dtype=torch.int32).cuda()
    sig_out = torch.empty((N, _lib.SIG_BYTES), dtype=torch.uint8, device="cuda")
    stream = _lib.current_stream_ptr(frames.device)
    rng = np.random.default_rng(1)
    sig_host = rng.integers(0, 256, (ROWS, _lib.SIG_BYTES), dtype=np.uint8)
    owner_host = np.repeat(np.arange(TRACKS, dtype=np.int32), ROWS // TRACKS)
    perm = rng.permutation(ROWS)
    sig, owner = torch.as_tensor(sig_host).cuda(), torch.as_tensor(owner_host).cuda()
    sig_sh, owner_sh = torch.as_tensor(sig_host[perm]).cuda(), torch.as_tensor(owner_host[perm]).cuda()
    dist = torch.empty((TRACKS, TRACKS), dtype=torch.int32, device="cuda")
    model = build_model()
    eps = synth.make_eps(GROUP, name="persons_timing").cuda()

    def signature():
        _lib.check(lib.gcv_face_signature(frames.data_ptr(), NF, H, W, bd.data_ptr(), N, sig_out.data_ptr(), stream),
                   "gcv_face_signature")

    def link(s=sig, o=owner):
        _lib.check(lib.gcv_sig_link(s.data_ptr(), o.data_ptr(), ROWS, TRACKS, dist.data_ptr(), stream), "gcv_sig_link")

    def score():
        for g in range(0, N, GROUP):
            model(_lib.face_crop_preprocess(frames, boxes[g:g + GROUP], dtype=torch.float16), eps=eps)
    calls = dict(signature=signature, link=link, link_shuffled=lambda: link(sig_sh, owner_sh), score=score)
    res = {"shape": {"frames": [NF, H, W], "boxes": N, "face_sides": [180, 220], "score_group": GROUP, "link_rows": ROWS,
                     "link_tracks": TRACKS}, "steps": a.steps, "rounds": a.rounds, "ms": {k: [] for k in calls}}
    for _ in range(a.rounds):
        for k, call in calls.items():
            res["ms"][k].append(round(median_ms(call, a.steps), 4))
    res["median_ms"] = {k: sorted(v)[len(v) // 2] for k, v in res["ms"].items()}
    res["over_score"] = {k: round(v / res["median_ms"]["score"], 5) for k, v in res["median_ms"].items() if k != "score"}
    t0 = time.perf_counter()
    want = pu.sig_link_ref(sig_host, owner_host, TRACKS)
    res["link_numpy_s"] = round(time.perf_counter() - t0, 3)
    link()
    same = bool(((dist.cpu().to(torch.int64) & pu.NONE).numpy() == want).all())
    link(sig_sh, owner_sh)
    res["link_equals_restatement"] = same and bool(((dist.cpu().to(torch.int64) & pu.NONE).numpy() == want).all())
    signature()
    res["rows_described"] = int(sig_out.any(1).sum())
    print(json.dumps(res))
    os.makedirs(os.path.dirname(a.out) or ".", exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
