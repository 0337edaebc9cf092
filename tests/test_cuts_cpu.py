"""Shot cuts without a GPU: ``track_boxes(cuts=...)`` against hand-written lists, the CPU restatement of the two device
entries (tests/cutsutil.py) on the three-shot video, and the host logic around them (``shot_cuts``,
``scan_frames(cuts=...)``) with ``_lib.frame_hist`` and ``_lib.hist_diff`` replaced by that restatement."""
import numpy as np
import pytest
import torch

from genconvit_amd import _lib
from genconvit_amd.model import pred_func
from tests import cutsutil as cu
from tests import followutil as fu
from tests import scanutil as su

torch.set_grad_enabled(False)


# ----------------------------------------------------------------------------- track_boxes(cuts=...)
def test_track_boxes_a_cut_ends_the_track_of_a_box_that_stays_put():
    box = lambda f: (f, 20, 90, 80, 30)
    seen = [box(f) for f in range(9)]
    assert pred_func.track_boxes(seen) == [seen]
    assert pred_func.track_boxes(seen, cuts=[5]) == [seen[:5], seen[5:]]
    assert pred_func.track_boxes(seen, cuts=[5, 6]) == [seen[:5], seen[5:6], seen[6:]]     # a one-frame flash
    tracks, anchors = pred_func.track_boxes(seen, cuts=[5], return_anchors=True)
    assert tracks == [seen[:5], seen[5:]] and anchors == [[True] * 5, [True] * 4]


def test_track_boxes_no_box_is_interpolated_across_a_cut():
    box = lambda f: (f, 20, 90, 80, 30)
    seen = [box(0), box(4), box(8)]
    assert pred_func.track_boxes(seen, max_gap=4) == [[box(f) for f in range(9)]]
    assert pred_func.track_boxes(seen, max_gap=4, cuts=[6]) == [[box(f) for f in range(5)], [box(8)]]
    assert pred_func.track_boxes(seen, max_gap=4, cuts=[4]) == [[box(0)], [box(f) for f in range(4, 9)]]     # l < c <= f
    assert pred_func.track_boxes(seen, max_gap=4, cuts=[9]) == [[box(f) for f in range(9)]]


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
TRACK_OUTPUTS = {                      # what tests/test_scan_cpu.py expects of some of them, literally
    0: [[(0, 10, 50, 50, 10), (1, 11, 51, 51, 11)], [(0, 10, 150, 50, 110), (1, 12, 152, 52, 112)]],
    5: [[(0, 10, 100, 50, 20), (1, 11, 103, 54, 20), (2, 12, 107, 57, 21), (3, 13, 110, 61, 21)]],
    8: [[(f, 10 + f, 60 + 2 * f, 50 + 2 * f, 20 + f) for f in range(9)]],
}


def test_track_boxes_without_cuts_is_unchanged():
    for n, (boxes, kw) in enumerate(TRACK_INPUTS):
        plain = pred_func.track_boxes(boxes, **kw)
        assert pred_func.track_boxes(boxes, cuts=None, **kw) == plain == pred_func.track_boxes(boxes, cuts=[], **kw)
        assert pred_func.track_boxes(boxes, cuts=[], return_anchors=True, **kw) == \
            pred_func.track_boxes(boxes, return_anchors=True, **kw)
        if n in TRACK_OUTPUTS:
            assert plain == TRACK_OUTPUTS[n]


# ----------------------------------------------------------------------------- the restatement
def test_scores_of_the_three_shot_video():
    """regions = 4: every score inside a shot below 0.1 (0.018 ... 0.040 here), both cuts above 0.5 (0.966 and 0.925)"""
    frames = cu.three_shot_video()
    assert frames.shape == (15, 90, 130, 3) and frames.dtype == np.uint8
    hist = cu.frame_hist_ref(frames, 4)
    assert hist.shape == (15, 16, 64) and (hist.sum(-1) == cu.region_pixels(90, 130, 4)[None]).all()
    assert cu.region_pixels(90, 130, 4).sum() == 90 * 130 and set(cu.region_pixels(90, 130, 4).tolist()) == {22 * 32, 22 * 33, 23 * 32, 23 * 33}
    dist = cu.hist_diff_ref(hist)
    assert dist.shape == (14, 16) and (dist <= 2 * cu.region_pixels(90, 130, 4)[None]).all() and (dist % 2 == 0).all()
    scores = cu.scores_ref(dist, 90, 130, 4)
    print("\nthree-shot scores:", np.round(scores, 3).tolist())
    inside = [s for p, s in enumerate(scores) if p + 1 not in cu.CUTS]
    assert len(inside) == 12 and max(inside) < 0.1 and 0.018 <= min(inside) and max(inside) <= 0.040
    assert scores[4] > 0.5 and scores[8] > 0.5 and round(scores[4], 3) == 0.966 and round(scores[8], 3) == 0.925
    # the patch moves, but never through more than half of the regions: with every region kept it would show
    every = dist.sum(1) / (2.0 * 90 * 130)
    assert (every[[p for p in range(14) if p + 1 not in cu.CUTS]] > np.array(inside)).all()


def test_scores_keep_the_smaller_half_with_ties_to_the_lower_region():
    # 2 x 2 regions of an 8 x 12 frame hold 24 pixels each; keep two
    assert cu.scores_ref([[48, 0, 10, 10]], 8, 12, 2).tolist() == [10 / 96]
    assert cu.scores_ref([[7]], 5, 5, 1).tolist() == [7 / 50]
    # unequal regions (5 x 7 at R = 2: 2 x 3, 2 x 4, 3 x 3, 3 x 4 pixels): the tie 4, 4 goes to regions 0 and 1
    assert cu.scores_ref([[4, 4, 4, 4]], 5, 7, 2).tolist() == [8 / (2 * (6 + 8))]


# ----------------------------------------------------------------------------- shot_cuts
@pytest.fixture
def spy(monkeypatch):
    """the two device entries are the restatement; every call is recorded"""
    calls = []

    def frame_hist(frames_u8, regions=4, out=None):
        calls.append(("hist", int(frames_u8.shape[0]), regions, out is not None))
        return cu.frame_hist_cpu(frames_u8, regions, out)

    def hist_diff(hist):
        calls.append(("diff", int(hist.shape[0])))
        return cu.hist_diff_cpu(hist)
    monkeypatch.setattr(_lib, "frame_hist", frame_hist)
    monkeypatch.setattr(_lib, "hist_diff", hist_diff)
    return calls


def test_shot_cuts_finds_both_cuts_in_any_grouping(spy):
    frames = cu.three_shot_video()
    want = cu.scores_ref(cu.hist_diff_ref(cu.frame_hist_ref(frames, 4)), 90, 130, 4)
    cuts, scores = pred_func.shot_cuts(frames, dev="cpu")
    assert cuts == cu.CUTS == [5, 9] and scores.dtype == np.float64 and scores.shape == (14,)
    assert (scores == want).all()
    assert spy == [("hist", 15, 4, True), ("diff", 15)]
    spy.clear()
    small = pred_func.shot_cuts(frames, max_frames=4, dev="cpu")
    assert spy == [("hist", 4, 4, True)] * 3 + [("hist", 3, 4, True), ("diff", 15)]           # consecutive groups, one diff
    tens = pred_func.shot_cuts(torch.as_tensor(frames), max_frames=128, dev="cpu")
    for other in (small, tens):
        assert other[0] == [5, 9] and (other[1] == want).all()
    # other thresholds and grids: the scores do not depend on the threshold, the cuts do
    assert pred_func.shot_cuts(frames, threshold=1.0, dev="cpu")[0] == []
    assert pred_func.shot_cuts(frames, threshold=0.95, dev="cpu")[0] == [5]
    assert pred_func.shot_cuts(frames, threshold=0.03, dev="cpu")[0] == [p + 1 for p in range(14) if want[p] >= 0.03]
    for regions in (1, 2, 8):
        cuts, scores = pred_func.shot_cuts(frames, regions=regions, dev="cpu")
        assert cuts == [5, 9]
        assert (scores == cu.scores_ref(cu.hist_diff_ref(cu.frame_hist_ref(frames, regions)), 90, 130, regions)).all()


def test_shot_cuts_of_one_frame_and_its_refusals(spy):
    frames = cu.three_shot_video()
    for few in (frames[:1], frames[:0], torch.as_tensor(frames[:1])):
        cuts, scores = pred_func.shot_cuts(few, dev="cpu")
        assert cuts == [] and scores.shape == (0,) and scores.dtype == np.float64
    for bad in (0, 0.0, -0.1, 1.01, 2):
        with pytest.raises(ValueError):
            pred_func.shot_cuts(frames, threshold=bad, dev="cpu")
    for bad in (0, 3, 16, 4.0, True):
        with pytest.raises(ValueError):
            pred_func.shot_cuts(frames, regions=bad, dev="cpu")
    with pytest.raises(ValueError):
        pred_func.shot_cuts(frames, max_frames=0, dev="cpu")
    with pytest.raises(_lib.GenConViTHipError):
        pred_func.shot_cuts(frames.astype(np.float32), dev="cpu")
    with pytest.raises(_lib.GenConViTHipError):
        pred_func.shot_cuts(frames[..., :2], dev="cpu")
    assert spy == []                                                            # nothing of this reached a launch
    assert pred_func.shot_cuts(frames[4:6], dev="cpu")[0] == [1]                # two frames, one pair, a cut


def test_the_bindings_refuse_host_tensors_and_bad_arguments_before_any_launch():
    """reaches no device: the checks come before the first call into the library's kernels"""
    frames = torch.as_tensor(cu.three_shot_video())
    for call in (lambda: _lib.frame_hist(frames), lambda: _lib.frame_hist(frames.numpy()),
                 lambda: _lib.hist_diff(torch.zeros((3, 16, 64), dtype=torch.int32))):
        with pytest.raises(_lib.GenConViTHipError):
            call()


# ----------------------------------------------------------------------------- scan_frames(cuts=...)
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


def _straddles(first, last, cuts):
    return any(first < c <= last for c in cuts)


def test_scan_frames_ends_the_tracks_at_the_cuts(spy, on_cpu):
    frames = cu.three_shot_video()
    boxes = [(f, *cu.FACE_BOX) for f in range(15)]
    kw = dict(boxes=boxes, window=3, stride=1, max_batch=4)
    plain = pred_func.scan_frames(frames, StandIn(), **kw)
    assert plain["tracks"] == [boxes] and "cuts" not in plain and "cut_scores" not in plain and spy == []
    assert any(_straddles(w[1], w[2], [5, 9]) for w in plain["windows"])        # what the cuts are for
    res = pred_func.scan_frames(frames, StandIn(), cuts=True, **kw)
    assert res["cuts"] == [5, 9] and res["tracks"] == [boxes[:5], boxes[5:9], boxes[9:]]
    assert res["boxes"] == boxes and res["track_offsets"] == [0, 5, 9, 15]
    assert spy == [("hist", 4, 4, True)] * 3 + [("hist", 3, 4, True), ("diff", 15)]           # max_batch is the group
    want = cu.scores_ref(cu.hist_diff_ref(cu.frame_hist_ref(frames, 4)), 90, 130, 4)
    assert res["cut_scores"].dtype == np.float64 and (res["cut_scores"] == want).all()
    assert [w[:3] for w in res["windows"]] == [(0, 0, 2), (0, 1, 3), (0, 2, 4), (1, 5, 7), (1, 6, 8),
                                               (2, 9, 11), (2, 10, 12), (2, 11, 13), (2, 12, 14)]
    assert not any(_straddles(w[1], w[2], res["cuts"]) for w in res["windows"])
    assert not any(_straddles(s[1], s[2], res["cuts"]) for s in res["segments"])
    assert sorted(res) == sorted(list(plain) + ["cuts", "cut_scores"])
    # the same crops in the same order: the scores of the frames do not change, the votes do
    assert torch.equal(res["frame_scores"], plain["frame_scores"]) and len(res["track_verdicts"]) == 3
    # the cuts given explicitly: the same result, and nothing is measured
    spy.clear()
    given = pred_func.scan_frames(frames, StandIn(), cuts=[9, 5], **kw)
    assert spy == [] and given["cuts"] == [5, 9] and "cut_scores" not in given
    for key in ("tracks", "boxes", "track_offsets", "windows", "segments", "track_verdicts", "verdict"):
        assert given[key] == res[key]
    assert torch.equal(given["frame_scores"], res["frame_scores"])
    assert torch.equal(given["window_means"], res["window_means"])
    # thresholds and grids are passed on
    assert pred_func.scan_frames(frames, StandIn(), cuts=True, cut_threshold=0.95, cut_regions=2, **kw)["cuts"] == \
        pred_func.shot_cuts(frames, 0.95, 2, dev="cpu")[0]
    none = pred_func.scan_frames(frames, StandIn(), cuts=[], **kw)
    assert none["cuts"] == [] and none["tracks"] == [boxes]


def test_scan_frames_refuses_bad_cuts_before_anything_runs(spy, on_cpu, monkeypatch):
    frames = cu.three_shot_video()
    kw = dict(boxes=[(f, *cu.FACE_BOX) for f in range(15)], window=3)
    monkeypatch.setattr(pred_func, "track_boxes", lambda *a, **k: pytest.fail("ran"))
    for bad in ([0], [15], [5, 20], [-1], [5.0], [5.5], ["5"], "59", [None], [True], False, 5):
        with pytest.raises(ValueError):
            pred_func.scan_frames(frames, StandIn(), cuts=bad, **kw)
    for bad in (dict(cut_threshold=0.0), dict(cut_threshold=1.5), dict(cut_regions=3), dict(cut_regions=16)):
        with pytest.raises(ValueError):
            pred_func.scan_frames(frames, StandIn(), cuts=True, **bad, **kw)
    assert spy == []


def test_scan_frames_no_follow_job_straddles_a_cut(spy, on_cpu, monkeypatch):
    """the detector on every second frame, ``follow=True``: without the cuts the boxes of frames 5 and 9 are matched
    against a template from another shot; with them no job has fa < c <= fb, and those two frames go unscored"""
    jobs = []

    def track_match(frames_u8, rows, grid=64, radius=16):
        rows = [tuple(int(v) for v in j) for j in rows]
        jobs.append(rows)
        return torch.as_tensor(fu.track_match_ref(frames_u8, rows, grid, radius))
    monkeypatch.setattr(_lib, "track_match", track_match)
    frames = torch.as_tensor(cu.three_shot_video())
    kw = dict(boxes=[(f, *cu.FACE_BOX) for f in range(0, 15, 2)], detect_every=2, window=3, follow=True, follow_grid=16,
              follow_radius=2, max_batch=128)
    plain = pred_func.scan_frames(frames, StandIn(), **kw)
    assert [len(t) for t in plain["tracks"]] == [15] and plain["follow"][:, 1].tolist() == [1, 3, 5, 7, 9, 11, 13]
    assert len(jobs) == 1 and len(jobs[0]) == 7                                 # all 15 frames are used: no remapping
    assert sum(_straddles(j[5], j[11], [5, 9]) for j in jobs[0]) == 2
    jobs.clear()
    res = pred_func.scan_frames(frames, StandIn(), cuts=True, **kw)
    assert res["cuts"] == [5, 9]
    assert [[b[0] for b in t] for t in res["tracks"]] == [[0, 1, 2, 3, 4], [6, 7, 8], [10, 11, 12, 13, 14]]
    assert res["follow"][:, :2].tolist() == [[0, 1], [0, 3], [1, 7], [2, 11], [2, 13]]
    used = sorted({b[0] for t in res["tracks"] for b in t})                      # the slab holds the frames the jobs read
    assert len(jobs) == 1 and len(jobs[0]) == 5
    for j in jobs[0]:
        fs, fa, fb = used[j[0]], used[j[5]], used[j[11]]
        assert fa < fs < fb and not _straddles(fa, fb, res["cuts"])
    assert not any(_straddles(w[1], w[2], res["cuts"]) for w in res["windows"])
