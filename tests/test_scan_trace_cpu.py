"""What ``pred_func.scan_frames`` hands to the library, launch by launch, without a GPU: every ``_lib`` binding the scan can
reach is replaced by a stand-in that first writes down what it was given — which source frames the slab holds, and the
integer rows and arguments — and then answers with the suite's CPU restatement.  The trace of a scan with every option
on, and the integer-valued parts of its result, are compared exactly with tests/golden/scan_trace.json: a change of the
host code that moves a row into another launch, uploads another frame or cuts the groups elsewhere shows here.

The fixture is written by hand, never by pytest: ``python tests/test_scan_trace_cpu.py --record``."""
import json
import os
import sys

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if REPO not in sys.path:
    sys.path.insert(0, REPO)

from genconvit_amd import _lib                              # noqa: E402
from genconvit_amd.model import pred_func                   # noqa: E402
from tests import cutsutil as cu                            # noqa: E402
from tests import extendutil as eu                          # noqa: E402
from tests import followutil as fu                          # noqa: E402
from tests import personutil as pu                          # noqa: E402
from tests import qualityutil as qu                         # noqa: E402
from tests import scanutil as su                            # noqa: E402
from tests import transutil as tu                           # noqa: E402

torch.set_grad_enabled(False)
FIXTURE = os.path.join(REPO, "tests", "golden", "scan_trace.json")
NF, H, W = 18, 96, 128
HARD_CUT, DISSOLVE, NEXT_SHOT = 5, (9, 13), 14
MISSED = ((0, 36), (8, 48), (16, 48))                       # (frame, face height): faces the detector did not find
N_CROPS = 21                                                # the rows of the video below that pass the quality gate


# ----------------------------------------------------------------------------- the video
def _video():
    """(frames, boxes): 18 frames of 96 x 128.  Frames 0-4 show tests/transutil.py's first look, a hard cut, 5-8 the second,
    9-13 a linear dissolve (a = k / 6) from frame 8's clean picture to frame 14's, 14-17 the third.  Two smooth patterns of
    tests/personutil.py, 48 x 44 and 36 x 32 pixels, move a few pixels a frame in the first shot (the small one is painted
    black in frame 3: the quality gate drops that row), the large one alone in the second, both in the third; +-6 noise
    per channel after the blending.  ``boxes``: what a detector that looks at every second frame would find, the frames
    inside the dissolve included.  Pixel (0, 0) of frame f holds f in its red channel: a slab tells which frames it is."""
    rng = np.random.default_rng(23)
    looks = tu._looks(H, W)
    big, small = eu.pattern(0, 48, 44).astype(np.float64), eu.pattern(1, 36, 32).astype(np.float64)
    where = {}                                              # frame -> [(pattern, top, left), ...]
    for k in range(5):
        where[k] = [(big, 20 + (0, 6, 6, 3, 6)[k], 10 + 3 * k), (small, 50, 80 + k)]
    for k in range(4):
        where[5 + k] = [(big, 30 + k, 60 - 2 * k)]
        where[14 + k] = [(small, 40, 20 + 2 * k), (big, 10 + k, 70)]

    def clean(f):
        pic = looks[0 if f < 5 else 1 if f < 9 else 2].copy()
        for patch, top, left in where[f]:
            pic[top:top + patch.shape[0], left:left + patch.shape[1]] = patch
        return pic
    pics = {f: clean(f) for f in where}
    if 3 in pics:
        patch, top, left = where[3][1]
        pics[3][top:top + patch.shape[0], left:left + patch.shape[1]] = 0.0
    for k in range(1, 6):
        pics[8 + k] = (1 - k / 6) * pics[8] + (k / 6) * pics[14]
        where[8 + k] = where[8]
    frames = np.stack([np.clip(pics[f] + rng.integers(-6, 7, size=pics[f].shape), 0, 255).astype(np.uint8) for f in range(NF)])
    frames[:, 0, 0, 0] = np.arange(NF)
    boxes = [(f, top, left + p.shape[1], top + p.shape[0], left) for f in range(0, NF, 2) for p, top, left in where[f]
             if (f, p.shape[0]) not in MISSED]
    return frames, boxes


def _eps():
    return torch.as_tensor(np.random.default_rng(5).integers(-2, 3, size=(N_CROPS, 4))).float()


# ----------------------------------------------------------------------------- the stand-ins
def _source(frames_u8):
    """the source frame numbers of a slab, from the tag in pixel (0, 0)"""
    return [int(v) for v in frames_u8[:, 0, 0, 0].tolist()]


def _rows(rows, width):
    return np.asarray(torch.as_tensor(rows).cpu() if torch.is_tensor(rows) else rows, dtype=np.int64).reshape(-1, width).tolist()


def _first_row(out, whole_row):
    """where in the whole video's buffer a group's ``out=`` rows start"""
    return None if out is None else [out.storage_offset() // whole_row, int(out.shape[0])]


def _fill(out, value):
    if out is None:
        return value
    out.copy_(value)
    return out


class Model(torch.nn.Module):
    """both networks' logits from the crop stand-in's five integers alone: net k gives (v, -v) with
    v = ((7 f + 3 top + left + k) % 9) - 4, plus the first entry of the crop's ``eps`` row"""
    net = "genconvit"

    def __init__(self, trace):
        super().__init__()
        self.k = torch.nn.Parameter(torch.tensor(1.0))
        self.trace = trace

    def forward(self, x, eps=None):
        rows = _rows(x, 5)
        self.trace.append(["model", rows, None if eps is None else _rows(eps, eps.shape[1])])
        base = torch.as_tensor([7 * f + 3 * top + left for f, top, _, _, left in rows])
        out = []
        for k in range(2):
            v = ((base + k) % 9 - 4).float() + (0.0 if eps is None else eps[:, 0].float())
            out.append(torch.stack((v, -v), 1))
        return torch.cat(out)


def _stand_ins(trace):
    def face_crop_preprocess(frames_u8, boxes, size=224, dtype=None):
        src, rows = _source(frames_u8), _rows(boxes, 5)
        trace.append(["face_crop_preprocess", src, rows, int(size), str(dtype)])
        return torch.as_tensor([(src[f], *box) for f, *box in rows], dtype=dtype or torch.float32).reshape(-1, 5)

    def vote_windows(logits, batch, nets, ranges):
        values = logits.double()
        assert torch.equal(values, values.round())
        trace.append(["vote_windows", _rows(values, 2), int(batch), int(nets), _rows(ranges, 2)])
        frame_p, mean2 = su.vote_windows_ref(logits, batch, nets, ranges)
        # six decimals: an exact tie between the two means is one on every CPU, whatever the order of its sums
        return (frame_p * 1e6).round().div(1e6).float(), (mean2 * 1e6).round().div(1e6).float()

    def track_match(frames_u8, jobs, grid=64, radius=16):
        rows = _rows(jobs, 17)
        trace.append(["track_match", _source(frames_u8), rows, int(grid), int(radius)])
        _lib._check_track_jobs("track_match", rows, *frames_u8.shape[:3], grid)
        return torch.as_tensor(fu.track_match_ref(frames_u8, rows, grid, radius))

    def track_chain(frames_u8, jobs, grid=64, radius=8):
        rows = _rows(jobs, 11)
        trace.append(["track_chain", _source(frames_u8), rows, int(grid), int(radius)])
        _lib._check_chain_jobs("track_chain", rows, *frames_u8.shape[:3], grid)
        return torch.as_tensor(eu.track_chain_ref(frames_u8, rows, grid, radius))

    def frame_hist(frames_u8, regions=4, out=None):
        trace.append(["frame_hist", _source(frames_u8), int(regions), _first_row(out, regions * regions * cu.BINS)])
        return _fill(out, torch.as_tensor(cu.frame_hist_ref(frames_u8, regions)))

    def frame_cells(frames_u8, grid=16, out=None):
        trace.append(["frame_cells", _source(frames_u8), int(grid), _first_row(out, grid * grid)])
        return _fill(out, torch.as_tensor(tu.frame_cells_ref(frames_u8, grid).astype(np.int32)))

    def hist_diff(hist):
        trace.append(["hist_diff", list(hist.shape), int(hist.long().sum())])
        return torch.as_tensor(cu.hist_diff_ref(hist).astype(np.int32))

    def hist_diff_lag(hist, lag):
        trace.append(["hist_diff_lag", list(hist.shape), int(hist.long().sum()), int(lag)])
        return torch.as_tensor(tu.hist_diff_lag_ref(hist, lag).astype(np.int32))

    def blend_fit(cells, lag):
        trace.append(["blend_fit", list(cells.shape), int(cells.long().sum()), int(lag)])
        return torch.as_tensor(tu.blend_fit_ref(cells, lag))

    def face_quality(frames_u8, boxes, grid=64):
        rows = _rows(boxes, 5)
        trace.append(["face_quality", _source(frames_u8), rows, int(grid)])
        _lib._check_quality_boxes("face_quality", rows, *frames_u8.shape[:3], grid)
        return torch.as_tensor(qu.face_quality_ref(frames_u8, rows, grid))

    def face_signature(frames_u8, boxes):
        rows = _rows(boxes, 5)
        trace.append(["face_signature", _source(frames_u8), rows])
        _lib._check_quality_boxes("face_signature", rows, *frames_u8.shape[:3], _lib.SIG_GRID)
        return torch.as_tensor(pu.face_signature_ref(frames_u8, rows))

    def sig_link(sig, owner, tracks):
        trace.append(["sig_link", list(sig.shape), int(sig.long().sum()), [int(o) for o in owner], int(tracks)])
        return torch.as_tensor(pu.sig_link_ref(sig, np.asarray(owner), tracks))
    return {f.__name__: f for f in (face_crop_preprocess, vote_windows, track_match, track_chain, frame_hist, frame_cells,
                                    hist_diff, hist_diff_lag, blend_fit, face_quality, face_signature, sig_link)}


# ----------------------------------------------------------------------------- one scan, as plain integers
def _plain(v):
    """tuples, arrays and tensors, also inside dicts, as nested lists of Python integers and bools"""
    if torch.is_tensor(v):
        v = v.cpu().numpy()
    if isinstance(v, np.ndarray):
        return v.tolist()
    if isinstance(v, dict):
        return {k: _plain(x) for k, x in v.items()}
    if isinstance(v, (list, tuple)):
        return [_plain(x) for x in v]
    return v.item() if isinstance(v, np.generic) else v


def _scan(frames, boxes, max_batch, patch):
    """(trace, the integer-valued parts of the result) of one scan with every option on"""
    trace = []
    for name, f in _stand_ins(trace).items():
        patch(_lib, name, f)
    res = pred_func.scan_frames(frames, Model(trace), boxes=boxes, detect_every=2, window=3, stride=2, max_batch=max_batch,
                                eps=_eps(), follow=True, follow_grid=16, follow_radius=4, cuts=True, transitions=True,
                                transition_args=dict(grid=16, lags=(4, 8)), quality=True, quality_args=dict(grid=16),
                                persons=True, extend=True, extend_args=dict(grid=16, radius=4, steps=4))
    q, p = res["quality"], res["persons"]
    part = {"keys": sorted(res), "tracks": res["tracks"], "boxes": res["boxes"], "track_offsets": res["track_offsets"],
            "windows": [w[:3] for w in res["windows"]], "segments": [s[:3] for s in res["segments"]], "cuts": res["cuts"],
            "transitions": res["transitions"], "follow": res["follow"], "extend": res["extend"],
            "quality": {"raw": q["raw"], "kept": q["kept"], "track_map": q["track_map"]},
            "persons": {k: p[k] for k in ("tracks", "of_track", "distance", "rows", "measured")}}
    return json.loads(json.dumps(_plain({"trace": trace, "result": part})))


CASES = {"groups of 3": 3, "one group": 1024}


def _record():
    class Patch:
        def __init__(self):
            self.saved = []

        def __call__(self, obj, name, value):
            self.saved.append((obj, name, getattr(obj, name)))
            setattr(obj, name, value)
    patch = Patch()
    frames, boxes = _video()
    try:
        got = {case: _scan(frames, boxes, max_batch, patch) for case, max_batch in CASES.items()}
    finally:
        for obj, name, value in reversed(patch.saved):
            setattr(obj, name, value)
    with open(FIXTURE, "w") as f:
        f.write("{\n" + ",\n".join(f"{json.dumps(case)}: {{\n" + ",\n".join(
            f" {json.dumps(k)}: " + (json.dumps(v, separators=(",", ":")) if k == "result" else
                                     "[\n" + ",\n".join("  " + json.dumps(t, separators=(",", ":")) for t in v) + "\n ]")
            for k, v in part.items()) + "\n}" for case, part in got.items()) + "\n}\n")
    print(f"{FIXTURE}: {os.path.getsize(FIXTURE)} bytes, " +
          ", ".join(f"{case}: {len(part['trace'])} calls, {len(part['result']['boxes'])} crops" for case, part in got.items()))


# ----------------------------------------------------------------------------- the tests
def _same(got, want):
    assert [t[0] for t in got["trace"]] == [t[0] for t in want["trace"]]
    for k, (a, b) in enumerate(zip(got["trace"], want["trace"])):
        assert a == b, f"call {k} ({a[0]})"
    assert sorted(got["result"]) == sorted(want["result"])
    for key in want["result"]:
        assert got["result"][key] == want["result"][key], key


def _wanted():
    with open(FIXTURE) as f:
        return json.load(f)


def test_the_video_exercises_every_stage_in_several_groups():
    want = _wanted()["groups of 3"]
    calls = [t[0] for t in want["trace"]]
    for name in _stand_ins([]):
        assert calls.count(name) >= 1, name
    for name in ("face_crop_preprocess", "model", "track_match", "track_chain", "frame_hist", "frame_cells", "face_quality",
                 "face_signature"):
        assert calls.count(name) >= 3, name
    assert calls.count("vote_windows") == 2 and calls.count("sig_link") == 1 and calls.count("hist_diff") == 1
    res = want["result"]
    assert res["cuts"] == [HARD_CUT] and res["transitions"] == [list(DISSOLVE)]
    assert len(res["boxes"]) == N_CROPS == sum(res["quality"]["kept"]) < len(res["quality"]["kept"])
    assert len(res["follow"]) >= 4 and len(res["extend"]) >= 4 and len(res["segments"]) >= 1
    assert any(len(p) > 1 for p in res["persons"]["tracks"])
    # a slab never holds more than the group's frames, and the crops of one launch never more than max_batch
    assert all(len(t[1]) <= 3 for t in want["trace"] if t[0] not in ("model", "hist_diff", "hist_diff_lag", "blend_fit",
                                                                    "sig_link", "vote_windows"))
    one = [t[0] for t in _wanted()["one group"]["trace"]]
    assert all(one.count(name) == 1 for name in ("face_crop_preprocess", "track_match", "face_quality", "face_signature"))


def test_a_scan_of_host_frames_issues_the_recorded_launches(monkeypatch):
    frames, boxes = _video()
    want = _wanted()["groups of 3"]
    _same(_scan(frames, boxes, CASES["groups of 3"], monkeypatch.setattr), want)
    _same(_scan(torch.as_tensor(frames), boxes, CASES["groups of 3"], monkeypatch.setattr), want)


def test_a_scan_in_one_group_issues_the_recorded_launches(monkeypatch):
    frames, boxes = _video()
    _same(_scan(frames, boxes, CASES["one group"], monkeypatch.setattr), _wanted()["one group"])


if __name__ == "__main__":
    if sys.argv[1:] != ["--record"]:
        raise SystemExit("usage: python tests/test_scan_trace_cpu.py --record")
    _record()
