"""The host side of the whole-video scan (``pred_func.window_ranges``, ``track_boxes``, ``scan_frames``, ``scan_video``)
without a GPU: the two device entry points are replaced by their CPU restatements (tests/scanutil.py) and the model by a
stand-in whose logits are a known function of each crop's mean colour, so every expected value below is written by hand."""
import numpy as np
import pytest
import torch

from genconvit_amd import _lib
from genconvit_amd.model import pred_func
from tests import scanutil as su

torch.set_grad_enabled(False)


# ----------------------------------------------------------------------------- window_ranges
def test_window_ranges_window_15_stride_1():
    wr = pred_func.window_ranges
    assert wr(0, 15, 1) == []
    assert wr(1, 15, 1) == [(0, 1)]
    assert wr(14, 15, 1) == [(0, 14)]
    assert wr(15, 15, 1) == [(0, 15)]
    assert wr(16, 15, 1) == [(0, 15), (1, 16)]
    assert wr(37, 15, 1) == [(s, s + 15) for s in range(23)] and wr(37, 15, 1)[-1] == (22, 37)


def test_window_ranges_appends_the_tail_only_when_the_stride_misses_it():
    assert pred_func.window_ranges(37, 15, 7) == [(0, 15), (7, 22), (14, 29), (21, 36), (22, 37)]
    assert pred_func.window_ranges(30, 15, 15) == [(0, 15), (15, 30)]
    assert pred_func.window_ranges(-3, 15, 15) == []


@pytest.mark.parametrize("window,stride", [(0, 1), (15, 0), (-1, 1), (15, -2)])
def test_window_ranges_rejects_bad_arguments(window, stride):
    with pytest.raises(ValueError):
        pred_func.window_ranges(20, window, stride)


# ----------------------------------------------------------------------------- track_boxes
def test_track_boxes_follows_two_faces_that_swap_row_order():
    a0, b0 = (0, 10, 50, 50, 10), (0, 10, 150, 50, 110)
    a1, b1 = (1, 11, 51, 51, 11), (1, 12, 152, 52, 112)
    assert pred_func.track_boxes([a0, b0, b1, a1]) == [[a0, a1], [b0, b1]]


def test_track_boxes_a_face_gone_for_longer_than_max_gap_comes_back_as_a_new_track():
    box = lambda f: (f, 20, 90, 70, 40)
    assert pred_func.track_boxes([box(0), box(1), box(4), box(5)], max_gap=2) == [[box(0), box(1)], [box(4), box(5)]]
    assert len(pred_func.track_boxes([box(0), box(1), box(4), box(5)], max_gap=3)) == 1


def test_track_boxes_the_higher_iou_takes_the_track_and_the_other_opens_one():
    t = (0, 0, 100, 100, 0)
    far, near = (1, 0, 100, 100, 40), (1, 0, 100, 100, 10)        # IoU 0.6 and 0.9 with t; the lower one comes first
    assert pred_func.track_boxes([t, far, near]) == [[t, near], [far]]
    assert pred_func.track_boxes([t, far, near], iou=0.95) == [[t], [far], [near]]


def test_track_boxes_fills_a_gap_of_three_with_rounded_interpolation():
    a, b = (0, 10, 100, 50, 20), (3, 13, 110, 61, 21)
    want = [a, (1, 11, 103, 54, 20), (2, 12, 107, 57, 21), b]     # floor(a + (b - a) k / 3 + 0.5) per coordinate
    assert pred_func.track_boxes([a, b], max_gap=3) == [want]
    assert pred_func.track_boxes([a, b], max_gap=2) == [[a], [b]]
    c, d = (0, 10, 100, 50, 20), (2, 13, 101, 53, 20)             # halves round up: 11.5 -> 12, 100.5 -> 101, 51.5 -> 52
    assert pred_func.track_boxes([c, d], max_gap=2) == [[c, (1, 12, 101, 52, 20), d]]


def test_track_boxes_a_detection_every_fourth_frame():
    seen = [(0, 10, 60, 50, 20), (4, 14, 68, 58, 24), (8, 18, 76, 66, 28)]
    want = [(f, 10 + f, 60 + 2 * f, 50 + 2 * f, 20 + f) for f in range(9)]
    assert pred_func.track_boxes(seen, max_gap=4) == [want]
    assert pred_func.track_boxes(seen, max_gap=1) == [[b] for b in seen]


# ----------------------------------------------------------------------------- scan_frames
class StandIn(torch.nn.Module):
    """logits = (k m, -k m) with m the crop's mean normalised red: a dark-red crop votes REAL (column 1), a bright-red one
    FAKE (column 0).  "genconvit" stacks a second network with another k, shifted by the first ``eps`` entry of each row."""

    def __init__(self, net):
        super().__init__()
        self.net = net
        self.k = torch.nn.Parameter(torch.tensor([4.0, 2.0]))
        self.calls = []

    def forward(self, x, eps=None):
        self.calls.append(x.shape[0])
        m = x[:, 0].float().mean((1, 2))
        one = lambda k: torch.stack((k * m, -k * m), 1)
        if self.net == "ed":
            return one(self.k[0])
        shift = 0.0 if eps is None else 0.25 * eps[:, :1]
        return torch.cat((one(self.k[0]), one(self.k[1]) + shift))


BOX_A, BOX_B = (10, 60, 50, 20), (40, 140, 80, 100)               # (top, right, bottom, left)


def _scene():
    """20 frames of 90 x 160, grey, two dark-red faces; face B turns bright red on frames 8 - 14."""
    frames = np.full((20, 90, 160, 3), 128, dtype=np.uint8)
    frames[:, 10:50, 20:60, 0] = 10
    frames[:, 40:80, 100:140, 0] = 10
    frames[8:15, 40:80, 100:140, 0] = 250
    boxes = [(f, *b) for f in range(20) for b in (BOX_A, BOX_B)]
    return frames, boxes


@pytest.fixture
def on_cpu(monkeypatch):
    monkeypatch.setattr(_lib, "face_crop_preprocess", su.face_crop_preprocess_ref)

    def vote_windows(logits, batch, nets, ranges):
        frame_p, mean2 = su.vote_windows_ref(logits, batch, nets, ranges)
        return frame_p.float(), mean2.float()
    monkeypatch.setattr(_lib, "vote_windows", vote_windows)


def _pinned(model, eps):
    """``model`` for ``pred_vid``, which passes no eps: the forward sees the given rows."""
    class P(torch.nn.Module):
        def __init__(self):
            super().__init__()
            self.m = model

        def forward(self, x):
            return self.m(x, eps=eps)
    return P()


@pytest.mark.parametrize("net", ["ed", "genconvit"])
def test_scan_frames_finds_the_one_fake_segment(on_cpu, net):
    frames, boxes = _scene()
    model = StandIn(net)
    nets = 1 if net == "ed" else 2
    eps = torch.randn(40, 8, generator=torch.Generator().manual_seed(3)) if nets == 2 else None
    res = pred_func.scan_frames(frames, model, boxes=boxes, window=5, stride=1, max_batch=128, eps=eps)
    assert res["tracks"] == [[(f, *BOX_A) for f in range(20)], [(f, *BOX_B) for f in range(20)]]
    assert res["boxes"] == res["tracks"][0] + res["tracks"][1] and res["track_offsets"] == [0, 20, 40]
    # a window of 5 is FAKE when at least 3 of its frames lie in 8 ... 14: the starts 6 ... 12 of track 1
    assert [w[:4] for w in res["windows"]] == [(t, s, s + 4, 0 if t == 1 and 6 <= s <= 12 else 1)
                                                for t in (0, 1) for s in range(16)]
    assert len(res["segments"]) == 1 and res["segments"][0][:3] == (1, 6, 16)
    peak = max(w[4] for w in res["windows"] if w[3] == 0)
    assert res["segments"][0][3] == peak and peak > 0.9
    assert tuple(res["window_means"].shape) == (32, 2) and tuple(res["frame_scores"].shape) == (40, 2)
    # the scores are those of one forward over all crops in (track, frame) order
    df = su.face_crop_preprocess_ref(frames, res["boxes"])
    want_p, _ = su.vote_windows_ref(model(df, eps=eps), 40, nets, [])
    assert (res["frame_scores"].double() - want_p).abs().max().item() <= 1e-6
    # verdicts: pred_vid on the same crops
    y, y_val = pred_func.pred_vid(df, _pinned(model, eps))
    assert res["verdict"][0] == y and abs(res["verdict"][1] - y_val) <= 1e-6
    for t in (0, 1):
        e = None if eps is None else eps[20 * t:20 * t + 20]
        y, y_val = pred_func.pred_vid(df[20 * t:20 * t + 20], _pinned(model, e))
        assert res["track_verdicts"][t][0] == y == 1 and abs(res["track_verdicts"][t][1] - y_val) <= 1e-6


@pytest.mark.parametrize("net", ["ed", "genconvit"])
def test_scan_frames_is_the_same_in_small_groups_and_for_tensor_frames(on_cpu, net):
    frames, boxes = _scene()
    eps = torch.randn(40, 8, generator=torch.Generator().manual_seed(3)) if net == "genconvit" else None
    kw = dict(boxes=boxes, window=5, stride=1, eps=eps)
    model = StandIn(net)
    base = pred_func.scan_frames(frames, model, max_batch=128, **kw)
    assert model.calls == [40]
    model.calls.clear()
    small = pred_func.scan_frames(frames, model, max_batch=5, **kw)
    assert model.calls == [5] * 8
    tens = pred_func.scan_frames(torch.as_tensor(frames), model, max_batch=128, **kw)
    for other in (small, tens):
        for key in ("tracks", "boxes", "track_offsets"):
            assert other[key] == base[key]
        assert [s[:3] for s in other["segments"]] == [s[:3] for s in base["segments"]] == [(1, 6, 16)]
        assert [w[:4] for w in other["windows"]] == [w[:4] for w in base["windows"]]
        assert other["verdict"][0] == base["verdict"][0] and abs(other["verdict"][1] - base["verdict"][1]) <= 1e-6
        assert [v[0] for v in other["track_verdicts"]] == [v[0] for v in base["track_verdicts"]]
        assert (other["frame_scores"] - base["frame_scores"]).abs().max().item() <= 1e-6
        assert (other["window_means"] - base["window_means"]).abs().max().item() <= 1e-6


def test_scan_frames_detects_on_every_second_frame_and_keeps_all_faces(on_cpu):
    frames, _ = _scene()
    seen = []

    def locate(fr):
        seen.append(len(fr))
        return [(i, *b) for i in range(len(fr)) for b in (BOX_B, BOX_A)]       # 20 faces on 10 frames: all are kept
    res = pred_func.scan_frames(frames, StandIn("ed"), locate=locate, detect_every=2, window=5, stride=1)
    assert seen == [10]
    assert res["tracks"] == [[(f, *BOX_B) for f in range(19)], [(f, *BOX_A) for f in range(19)]]
    assert [s[:3] for s in res["segments"]] == [(0, 6, 16)]


def test_scan_frames_default_detector_keeps_every_face_to_the_last_frame(on_cpu, monkeypatch):
    """the default path: ``face_locations`` behind stand-ins for face_recognition / dlib that find two faces on every
    frame.  ``face_rec``'s cut at len(frames) boxes would stop after half the video; the scan must reach the last frame."""
    import sys
    import types
    calls = []

    def locations(bgr, number_of_times_to_upsample=1, model="hog"):
        assert isinstance(bgr, np.ndarray) and bgr.shape == (90, 160, 3) and model == "hog"
        calls.append(int(bgr[0, 0, 1]))
        return [BOX_A, BOX_B]
    monkeypatch.setitem(sys.modules, "dlib", types.SimpleNamespace(DLIB_USE_CUDA=False))
    monkeypatch.setitem(sys.modules, "face_recognition", types.SimpleNamespace(face_locations=locations))
    frames, _ = _scene()
    assert len(pred_func.face_locations(frames)) == 20 and pred_func.face_locations(frames)[-1][0] == 9      # as before
    assert len(pred_func.face_locations(frames, keep_all=True)) == 40
    for fr in (frames, torch.as_tensor(frames)):                   # the detector gets numpy frames either way
        res = pred_func.scan_frames(fr, StandIn("ed"), window=5, stride=1)
        assert [len(t) for t in res["tracks"]] == [20, 20] and res["tracks"][0][-1] == (19, *BOX_A)
        assert res["tracks"][1][-1] == (19, *BOX_B) and [s[:3] for s in res["segments"]] == [(1, 6, 16)]
    res = pred_func.scan_frames(frames, StandIn("ed"), detect_every=3, window=5, stride=1)
    assert [len(t) for t in res["tracks"]] == [19, 19] and res["tracks"][1][-1] == (18, *BOX_B)    # detector frames 0, 3 ... 18


def test_scan_frames_uploads_only_the_frames_its_crops_lie_on(on_cpu, monkeypatch):
    """two faces 19 frames apart in one group: the slab is those two frames, not the 20 between them"""
    frames, _ = _scene()
    slabs = []

    def crop(slab, boxes, **kw):
        slabs.append((tuple(slab.shape), [b[0] for b in boxes]))
        return su.face_crop_preprocess_ref(slab, boxes, **kw)
    monkeypatch.setattr(_lib, "face_crop_preprocess", crop)
    boxes = [(0, *BOX_A), (19, *BOX_B), (19, *BOX_A)]
    res = pred_func.scan_frames(frames, StandIn("ed"), boxes=boxes, window=5)
    assert slabs == [((2, 90, 160, 3), [0, 1, 1])] and len(res["tracks"]) == 3
    want = su.vote_windows_ref(StandIn("ed")(su.face_crop_preprocess_ref(frames, res["boxes"])), 3, 1, [])[0]
    assert (res["frame_scores"].double() - want).abs().max().item() <= 1e-6


def test_scan_frames_without_a_face_launches_nothing(on_cpu, monkeypatch):
    def boom(*a, **k):
        raise AssertionError("launched")
    monkeypatch.setattr(_lib, "face_crop_preprocess", boom)
    monkeypatch.setattr(_lib, "vote_windows", boom)
    frames, _ = _scene()
    model = StandIn("genconvit")
    for kw in (dict(boxes=[]), dict(locate=lambda fr: [])):
        res = pred_func.scan_frames(frames, model, **kw)
        assert res["verdict"] == (None, None) and model.calls == []
        assert res["tracks"] == [] and res["boxes"] == [] and res["track_offsets"] == [0]
        assert res["windows"] == [] and res["track_verdicts"] == [] and res["segments"] == []
        assert tuple(res["frame_scores"].shape) == (0, 2) and tuple(res["window_means"].shape) == (0, 2)


def test_scan_frames_rejects_a_box_outside_its_frame(on_cpu):
    frames, _ = _scene()
    with pytest.raises(_lib.GenConViTHipError):
        pred_func.scan_frames(frames, StandIn("ed"), boxes=[(0, 10, 170, 50, 20)])
    with pytest.raises(ValueError):
        pred_func.scan_frames(frames, StandIn("ed"), boxes=[(0, *BOX_A)], window=0)


# ----------------------------------------------------------------------------- scan_video
def test_scan_video_reads_every_kth_frame_and_reports_the_source_numbers(on_cpu, monkeypatch):
    video = np.zeros((50, 90, 160, 3), dtype=np.uint8)
    video[:, :, :, 1] = np.arange(50, dtype=np.uint8)[:, None, None]          # frame i is green = i
    video[:, 10:50, 20:60, 0] = 250

    def read(vid, select):
        assert vid == "clip.mp4"
        index = select(len(video))
        return video[index], index
    monkeypatch.setattr(pred_func, "_read_frames", read)
    got = {}
    scan = pred_func.scan_frames

    def spy(frames, model, **kw):
        got["frames"], got["kw"] = frames, kw
        return scan(frames, model, **kw)
    monkeypatch.setattr(pred_func, "scan_frames", spy)
    model = StandIn("ed")
    res = pred_func.scan_video("clip.mp4", model, every=3, max_frames=5, boxes=[(f, *BOX_A) for f in range(5)], window=2)
    assert res["frame_index"] == [0, 3, 6, 9, 12] and got["frames"][:, 0, 0, 1].tolist() == [0, 3, 6, 9, 12]
    assert got["kw"] == dict(boxes=[(f, *BOX_A) for f in range(5)], window=2)
    assert res["segments"] == [(0, 0, 4, res["segments"][0][3])] and res["verdict"][0] == 0
    assert pred_func.scan_video("clip.mp4", model, every=7, boxes=[])["frame_index"] == list(range(0, 50, 7))
    assert pred_func.scan_video("clip.mp4", model, max_frames=4, boxes=[])["frame_index"] == [0, 1, 2, 3]
    with pytest.raises(ValueError):
        pred_func.scan_video("clip.mp4", model, every=0)
