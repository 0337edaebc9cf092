"""Following a face between detector frames, without a GPU: the CPU restatement of ``gcv_track_match``
(tests/followutil.py) on cases whose answers are known, and the host logic around it (``track_boxes(return_anchors=True)``,
``follow_tracks``, ``scan_frames(follow=True)``) with ``_lib.track_match`` replaced by that restatement."""
import numpy as np
import pytest
import torch

from genconvit_amd import _lib
from genconvit_amd.model import pred_func
from tests import followutil as fu
from tests import scanutil as su

torch.set_grad_enabled(False)


# ----------------------------------------------------------------------------- the restatement
def test_path_case_recovers_the_curved_motion():
    frames, jobs, priors = fu.path_case()
    boxes = pred_func.track_boxes([jobs[0][5:10], jobs[0][11:16]], iou=0.05, max_gap=4)[0]
    assert [(b[1], b[4]) for b in boxes[1:4]] == priors == [(23, 38), (26, 45), (29, 53)]
    out = fu.track_match_ref(frames, jobs, 16, 4)
    assert out.dtype == np.int32 and out.shape == (3, 4)
    got = [(p[0] + int(o[0]), p[1] + int(o[1])) for p, o in zip(priors, out)]
    assert got == fu.PATH_FOLLOWED == [(29, 35), (32, 40), (32, 50)]
    assert got[:2] == fu.PATH_TOPLEFT[1:3] and fu.PATH_TOPLEFT[3] == (33, 50)      # the third: one pixel, a cell is 3 high
    assert out[1, 2] == 0
    assert (out[:, 2] < out[:, 3]).all()


def test_flat_frames_stay_where_they_are():
    frames = np.empty((2, 64, 80, 3), dtype=np.uint8)
    frames[0], frames[1] = (10, 200, 30), (10, 200, 30)
    jobs = [(1, 20, 50, 40, 20, 0, 5, 60, 37, 11, 1, 1, 30, 70, 64, 30, 3)]
    assert fu.track_match_ref(frames, jobs, 16, 5).tolist() == [[0, 0, 0, 0]]


@pytest.mark.parametrize("corner", ["top left", "top right", "bottom left", "bottom right"])
def test_a_prior_in_the_corner_never_leaves_the_frame(corner):
    rng = np.random.default_rng(8)
    H, W, h, w = 70, 90, 37, 33
    frames = rng.integers(0, 256, (2, H, W, 3), dtype=np.uint8)
    top = 0 if "top" in corner else H - h
    left = 0 if "left" in corner else W - w
    jobs = [(1, top, left + w, top + h, left, 0, 10, 60, 50, 20, 2, 0, 20, 80, 60, 40, 1)]
    for grid, radius in ((16, 8), (16, 32), (32, 1)):
        oy, ox, cost, cost0 = fu.track_match_ref(frames, jobs, grid, radius)[0]
        assert 0 <= top + oy and top + oy + h <= H and 0 <= left + ox and left + ox + w <= W
        assert cost <= cost0


def test_the_cells_of_a_displaced_box_tile_it():
    for grid in (16, 32, 64):
        for h in range(16, 201):
            for d in range(-32, 33):
                assert fu.edge(grid + d, h, grid) - fu.edge(d, h, grid) == h


# ----------------------------------------------------------------------------- track_boxes(return_anchors=True)
TRACK_INPUTS = [                       # the inputs of tests/test_scan_cpu.py: (boxes, keywords)
    ([(0, 10, 50, 50, 10), (0, 10, 150, 50, 110), (1, 12, 152, 52, 112), (1, 11, 51, 51, 11)], {}),
    ([(f, 20, 90, 70, 40) for f in (0, 1, 4, 5)], dict(max_gap=2)),
    ([(f, 20, 90, 70, 40) for f in (0, 1, 4, 5)], dict(max_gap=3)),
    ([(0, 0, 100, 100, 0), (1, 0, 100, 100, 40), (1, 0, 100, 100, 10)], {}),
    ([(0, 0, 100, 100, 0), (1, 0, 100, 100, 40), (1, 0, 100, 100, 10)], dict(iou=0.95)),
    ([(0, 10, 100, 50, 20), (3, 13, 110, 61, 21)], dict(max_gap=3)),
    ([(0, 10, 100, 50, 20), (3, 13, 110, 61, 21)], dict(max_gap=2)),
    ([(0, 10, 100, 50, 20), (2, 13, 101, 53, 20)], dict(max_gap=2)),
    ([(0, 10, 60, 50, 20), (4, 14, 68, 58, 24), (8, 18, 76, 66, 28)], dict(max_gap=4)),
    ([(0, 10, 60, 50, 20), (4, 14, 68, 58, 24), (8, 18, 76, 66, 28)], dict(max_gap=1)),
    ([], {}),
]


def test_track_boxes_anchor_flags_mark_exactly_the_input_rows():
    for boxes, kw in TRACK_INPUTS:
        plain = pred_func.track_boxes(boxes, **kw)
        tracks, anchors = pred_func.track_boxes(boxes, return_anchors=True, **kw)
        assert tracks == plain == pred_func.track_boxes(boxes, return_anchors=False, **kw)
        assert [len(a) for a in anchors] == [len(t) for t in tracks]
        assert all(type(v) is bool for a in anchors for v in a)
        seen = [b for t, a in zip(tracks, anchors) for b, d in zip(t, a) if d]
        assert sorted(seen) == sorted(tuple(b) for b in boxes)
    tracks, anchors = pred_func.track_boxes(*TRACK_INPUTS[8][:1], max_gap=4, return_anchors=True)
    assert anchors == [[True, False, False, False, True, False, False, False, True]]
    assert tracks == [[(f, 10 + f, 60 + 2 * f, 50 + 2 * f, 20 + f) for f in range(9)]]


# ----------------------------------------------------------------------------- follow_tracks
@pytest.fixture
def spy(monkeypatch):
    """``_lib.track_match`` is the restatement; every call is recorded as (frames of the slab, job rows, grid, radius)"""
    calls = []

    def track_match(frames_u8, jobs, grid=64, radius=16):
        jobs = [tuple(int(v) for v in j) for j in jobs]
        calls.append((frames_u8.shape[0], jobs, grid, radius))
        _lib._check_track_jobs("track_match", jobs, *frames_u8.shape[:3], grid)
        return torch.as_tensor(fu.track_match_ref(frames_u8, jobs, grid, radius))
    monkeypatch.setattr(_lib, "track_match", track_match)
    return calls


def _path_tracks():
    frames, jobs, _ = fu.path_case()
    return frames, *pred_func.track_boxes([jobs[0][5:10], jobs[0][11:16]], iou=0.05, max_gap=4, return_anchors=True)


def test_follow_tracks_builds_the_jobs_and_moves_the_filled_boxes(spy):
    frames, tracks, anchors = _path_tracks()
    _, jobs, _ = fu.path_case()
    moved, follow = pred_func.follow_tracks(frames, tracks, anchors, grid=16, radius=4)
    assert spy == [(5, [tuple(j) for j in jobs], 16, 4)]                    # frames 0 .. 4 are all needed: no remapping
    assert [j[10] for j in spy[0][1]] == [3, 2, 1] and [j[16] for j in spy[0][1]] == [1, 2, 3]
    want = fu.track_match_ref(frames, jobs, 16, 4)
    assert follow.dtype == np.int32 and follow.shape == (3, 6)
    assert follow[:, 0].tolist() == [0, 0, 0] and follow[:, 1].tolist() == [1, 2, 3]
    assert (follow[:, 2:] == want).all()
    assert moved[0][0] == tracks[0][0] and moved[0][4] == tracks[0][4]      # detections stay
    assert [(b[1], b[4]) for b in moved[0][1:4]] == fu.PATH_FOLLOWED
    assert [(b[3] - b[1], b[2] - b[4]) for b in moved[0]] == [(48, 40)] * 5
    assert [(b[1], b[4]) for b in tracks[0][1:4]] == [(23, 38), (26, 45), (29, 53)]        # the input is not changed


def test_follow_tracks_leaves_small_faces_and_open_ends_interpolated(spy):
    frames, tracks, anchors = _path_tracks()
    assert pred_func.follow_tracks(frames, tracks, anchors, grid=64, radius=4)[1].shape == (0, 6) and spy == []   # 48 x 40 < 64
    moved, follow = pred_func.follow_tracks(frames, tracks, anchors, grid=64, radius=4)
    assert moved == tracks
    # a filled box before the first / after the last detection, or beside a detection that is too small: no job
    tr = [(f, 10, 60, 50, 20) for f in range(5)]
    for flags in ([False, True, True, True, False], [False, False, True, False, False]):
        assert pred_func.follow_tracks(frames, [tr], [flags], grid=16, radius=2)[1].shape == (0, 6)
    small = [(0, 10, 60, 50, 20), (1, 10, 60, 50, 20), (2, 10, 35, 50, 20)]                # anchor b is 15 wide
    assert pred_func.follow_tracks(frames, [small], [[True, False, True]], grid=16, radius=2)[1].shape == (0, 6)
    assert spy == []
    with pytest.raises(ValueError):
        pred_func.follow_tracks(frames, tracks, anchors, grid=48)
    with pytest.raises(ValueError):
        pred_func.follow_tracks(frames, tracks, anchors, radius=33)
    with pytest.raises(ValueError):
        pred_func.follow_tracks(frames, tracks, anchors, grid=16, max_frames=2)


def test_follow_tracks_groups_by_the_frames_a_group_needs(spy):
    """two faces seen on frames 0, 3, 6: with max_frames=3 a group is one (fa, fb, fs) triple, and the two tracks that share
    it go together; the slab holds those three frames and the rows index into it"""
    frames, det, _ = fu.two_face_video()
    det = [(d[0] * 3 // 4, *d[1:]) for d in det]                                           # the detections, on 0, 3, 6
    frames = frames[[0, 1, 2, 4, 5, 6, 8]]                                                 # any frames will do
    tracks, anchors = pred_func.track_boxes(det, iou=0.05, max_gap=3, return_anchors=True)
    assert [len(t) for t in tracks] == [7, 7]
    moved, follow = pred_func.follow_tracks(frames, tracks, anchors, grid=16, radius=2, max_frames=3)
    assert [c[0] for c in spy] == [3, 3, 3, 3] and all(len(c[1]) == 2 for c in spy)
    for call, (fa, fb, fs) in zip(spy, [(0, 3, 1), (0, 3, 2), (3, 6, 4), (3, 6, 5)]):
        for t, row in enumerate(call[1]):
            assert (row[5], row[0], row[11]) == (0, 1, 2)                                  # remapped: fa < fs < fb
            assert row[1:5] == tracks[t][fs][1:] and row[6:10] == tracks[t][fa][1:] and row[12:16] == tracks[t][fb][1:]
            assert (row[10], row[16]) == (fb - fs, fs - fa)
    one, follow1 = pred_func.follow_tracks(frames, tracks, anchors, grid=16, radius=2, max_frames=128)
    assert len(spy) == 5 and spy[4][0] == 7 and len(spy[4][1]) == 8                        # one group: all seven frames
    assert one == moved and (follow1 == follow).all()
    assert follow[:, :2].tolist() == [[t, f] for t in (0, 1) for f in (1, 2, 4, 5)]        # (track, frame) order
    mid, follow2 = pred_func.follow_tracks(frames, tracks, anchors, grid=16, radius=2, max_frames=4)
    assert [c[0] for c in spy[5:]] == [4, 4] and mid == moved                              # {0, 1, 2, 3} and {3, 4, 5, 6}
    assert (follow[4:, 2:4] == 0).all()                                                    # the static face


# ----------------------------------------------------------------------------- scan_frames(follow=True)
class StandIn(torch.nn.Module):
    """logits = (k m, -k m) with m the crop's mean normalised red (the stand-in of tests/test_scan_cpu.py, one network)"""
    net = "ed"

    def __init__(self):
        super().__init__()
        self.k = torch.nn.Parameter(torch.tensor(4.0))

    def forward(self, x, eps=None):
        m = x[:, 0].float().mean((1, 2))
        return torch.stack((self.k * m, -self.k * m), 1)


@pytest.fixture
def on_cpu(monkeypatch):
    monkeypatch.setattr(_lib, "face_crop_preprocess", su.face_crop_preprocess_ref)

    def vote_windows(logits, batch, nets, ranges):
        frame_p, mean2 = su.vote_windows_ref(logits, batch, nets, ranges)
        return frame_p.float(), mean2.float()
    monkeypatch.setattr(_lib, "vote_windows", vote_windows)


def test_scan_frames_follows_before_it_crops(spy, on_cpu, monkeypatch):
    frames, jobs, _ = fu.path_case()
    det = [jobs[0][5:10], jobs[0][11:16]]
    kw = dict(boxes=det, detect_every=4, iou=0.05, window=3)
    res = pred_func.scan_frames(frames, StandIn(), follow=True, follow_grid=16, follow_radius=4, **kw)
    assert [(b[1], b[4]) for b in res["tracks"][0]] == [fu.PATH_TOPLEFT[0]] + fu.PATH_FOLLOWED + [fu.PATH_TOPLEFT[4]]
    assert res["boxes"] == res["tracks"][0] and len(spy) == 1
    assert res["follow"].shape == (3, 6) and (res["follow"][:, 2:] == fu.track_match_ref(frames, jobs, 16, 4)).all()
    # the crops are those of the followed boxes
    want = su.vote_windows_ref(StandIn()(su.face_crop_preprocess_ref(frames, res["boxes"])), 5, 1, [])[0]
    assert (res["frame_scores"].double() - want).abs().max().item() <= 1e-6
    # off by default: today's keys, today's boxes, and the matcher is not called
    plain = pred_func.scan_frames(frames, StandIn(), **kw)
    assert len(spy) == 1 and "follow" not in plain
    assert sorted(plain) == sorted(k for k in res if k != "follow")
    assert [(b[1], b[4]) for b in plain["tracks"][0][1:4]] == [(23, 38), (26, 45), (29, 53)]
    # bad values raise before anything runs; without follow they are not looked at
    monkeypatch.setattr(pred_func, "track_boxes", lambda *a, **k: pytest.fail("ran"))
    for bad in (dict(follow_grid=20), dict(follow_radius=-1), dict(follow_radius=33)):
        with pytest.raises(ValueError):
            pred_func.scan_frames(frames, StandIn(), follow=True, **bad, **kw)


def test_scan_frames_follow_without_a_face(spy, on_cpu):
    frames, _, _ = fu.path_case()
    res = pred_func.scan_frames(frames, StandIn(), boxes=[], follow=True)
    assert res["verdict"] == (None, None) and res["follow"].shape == (0, 6) and spy == []


# ----------------------------------------------------------------------------- the binding's row checks
def test_the_binding_rejects_bad_rows_before_any_launch():
    ok = (1, 20, 60, 68, 20, 0, 20, 60, 68, 20, 1, 2, 20, 60, 68, 20, 1)
    check = lambda row, grid=16: _lib._check_track_jobs("t", [row], 3, 96, 128, grid)
    assert tuple(check(ok).shape) == (1, 17) and tuple(_lib._check_track_jobs("t", [], 3, 96, 128, 16).shape) == (0, 17)
    edit = lambda **kw: tuple(kw.get(str(i), v) for i, v in enumerate(ok))
    bad = [edit(**{"0": 3}), edit(**{"5": -1}), edit(**{"11": 3}),                         # frame indices
           edit(**{"3": 97}), edit(**{"7": 129}), edit(**{"12": -1}), edit(**{"15": -2}),  # outside the frame
           edit(**{"3": 35}), edit(**{"7": 35}), edit(**{"14": 30}),                       # a side below the grid
           edit(**{"10": 0, "16": 0}), edit(**{"10": -1, "16": 3}), edit(**{"10": 1000, "16": 25})]
    for row in bad:
        with pytest.raises(_lib.GenConViTHipError):
            check(row)
    with pytest.raises(_lib.GenConViTHipError):
        check(ok, grid=64)                                                                 # 48 x 40 boxes
    check(edit(**{"10": 1024, "16": 0}))
    check(edit(**{"10": 0, "16": 1}))
