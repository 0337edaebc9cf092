"""Fades and dissolves without a GPU: the CPU restatement of the three device entries and of the rule (tests/transutil.py)
on the synthetic videos, and the host logic around them (``shot_transitions``, ``scan_frames(transitions=...)``) with
``_lib.frame_cells``, ``_lib.blend_fit``, ``_lib.hist_diff_lag``, ``_lib.frame_hist`` and ``_lib.hist_diff`` replaced by that
restatement."""
import numpy as np
import pytest
import torch

from genconvit_amd import _lib
from genconvit_amd.model import pred_func
from tests import cutsutil as cu
from tests import scanutil as su
from tests import transutil as tu
from tests.test_cuts_cpu import StandIn

torch.set_grad_enabled(False)

_CACHE = {}


def _video():
    if "video" not in _CACHE:
        _CACHE["video"] = tu.transition_video()
        _CACHE["want"] = tu.transitions_ref(_CACHE["video"])
    return _CACHE["video"], _CACHE["want"]


# ----------------------------------------------------------------------------- the restatement
def _candidates(d, h_min=0.25, a_lo=0.1, a_hi=0.9, slack=0.05):
    """the spans that pass every test but the one on rho"""
    a = d["a"]
    return (d["scores"] >= h_min) & (((a >= a_lo) & (a <= a_hi)).sum(1) >= 2) & (a[:, 1:] >= a[:, :-1] - slack).all(1)


@pytest.mark.parametrize("grid", [16, 32])
def test_the_rule_finds_the_dissolve_and_the_fade(grid):
    """accepted spans: rho <= 0.038 and lagged scores >= 0.79; spans that pass every other test are rejected with rho >=
    0.058 — the margin around rho_max = 0.05 on this material"""
    frames = tu.transition_video()
    assert frames.shape == (38, 90, 130, 3) and frames.dtype == np.uint8
    got, info = tu.transitions_ref(frames, grid=grid)
    assert got == tu.TRANSITIONS == [(8, 13), (30, 34)] and sorted(info) == [4, 8]
    accepted, rejected, scores = [], [], []
    for lag, d in info.items():
        assert d["a"].shape == d["rho"].shape == (38 - lag, lag - 1) and d["scores"].shape == d["blend"].shape == (38 - lag,)
        assert d["blend"].any() and (d["rho"] >= -1e-12).all()
        cand = _candidates(d)
        assert (d["blend"] <= cand).all()
        accepted += d["rho"].max(1)[d["blend"]].tolist()
        rejected += d["rho"].max(1)[cand & ~d["blend"]].tolist()
        scores += d["scores"][d["blend"]].tolist()
    print(f"\ngrid {grid}: accepted rho <= {max(accepted):.4f}, rejected rho >= {min(rejected):.4f}, scores >= {min(scores):.3f}")
    assert max(accepted) <= 0.038 and min(rejected) >= 0.058 and min(scores) >= 0.79 >= 0.3
    # the hard cut at frame 22 is no transition, and the histograms alone would not do: spans across it score high
    assert info[4]["scores"][20] > 0.9 and not info[4]["blend"][18:22].any()


@pytest.mark.parametrize("step,bound", [(1, 0.19), (2, 0.29), (4, 0.40)])
def test_a_pan_is_no_transition(step, bound):
    """at one pixel a frame the lagged scores stay below h_min (<= 0.19 against >= 0.79 on the blend spans); faster pans pass
    h_min at lag 8 and are turned down by rho"""
    frames = tu.pan_video(step)
    assert frames.shape == (24, 90, 130, 3)
    for grid in (16, 32):
        got, info = tu.transitions_ref(frames, grid=grid)
        assert got == [] and not any(d["blend"].any() for d in info.values())
        assert max(d["scores"].max() for d in info.values()) <= bound
    if step == 1:
        assert bound < tu.DEFAULTS["h_min"]


def test_hard_cuts_alone_are_no_transition():
    for grid in (16, 32):
        got, info = tu.transitions_ref(cu.three_shot_video(), grid=grid)
        assert got == [] and info[4]["scores"].max() > 0.9


def test_the_restated_entries_on_small_inputs():
    frames = cu.noise_video()
    y = cu.luma(frames)
    for grid in (8, 16, 32):
        cells = tu.frame_cells_ref(frames, grid)
        assert cells.shape == (4, grid * grid) and (cells.sum(1) == y.sum((1, 2))).all()
    one = tu.frame_cells_ref(frames[:, :32, :32], 32)
    assert (one == y[:, :32, :32].reshape(4, -1)).all()                         # one pixel per cell
    cells = np.array([[0, 0, 0], [1, 2, 3], [2, 4, 6], [9, 9, 9]])              # frame 1 is halfway from 0 to 2
    assert tu.blend_fit_ref(cells, 2).tolist() == [[56, 28, 14], [149, 40, 14]]
    assert tu.blend_fit_ref(cells, 3).tolist() == [[243, 54, 108, 14, 56]]
    assert tu.blend_fit_ref(cells, 4).shape == (0, 7)
    assert tu.fit_terms([56, 28, 14], 2) == ([0.5], [0.0])
    assert tu.fit_terms([0, 0, 0], 2) == ([0.0], [float("inf")])
    big = tu.extreme_cells()
    fit = tu.blend_fit_ref(big, 3)
    assert fit.shape == (3, 5) and fit.max() > 2 ** 62 and fit.min() < -2 ** 58          # far beyond a float64's 2^53
    hist = cu.frame_hist_ref(cu.three_shot_video(), 2)
    assert (tu.hist_diff_lag_ref(hist, 1) == cu.hist_diff_ref(hist)).all()
    assert tu.hist_diff_lag_ref(hist, 15).shape == (0, 4) and tu.hist_diff_lag_ref(hist, 14).shape == (1, 4)
    assert tu.runs({3, 4, 5, 9, 11, 12}) == [(3, 5), (9, 9), (11, 12)] and tu.runs(set()) == []


# ----------------------------------------------------------------------------- shot_transitions
@pytest.fixture
def spy(monkeypatch):
    """the five device entries are the restatement; every call is recorded, the frames of a call as the object handed in"""
    calls = []

    def frame_hist(frames_u8, regions=4, out=None):
        calls.append(("hist", frames_u8, regions, out is not None))
        return cu.frame_hist_cpu(frames_u8, regions, out)

    def frame_cells(frames_u8, grid=16, out=None):
        calls.append(("cells", frames_u8, grid, out is not None))
        return tu.frame_cells_cpu(frames_u8, grid, out)

    def hist_diff(hist):
        calls.append(("diff", int(hist.shape[0])))
        return cu.hist_diff_cpu(hist)

    def hist_diff_lag(hist, lag):
        calls.append(("difflag", int(hist.shape[0]), lag))
        return tu.hist_diff_lag_cpu(hist, lag)

    def blend_fit(cells, lag):
        calls.append(("fit", int(cells.shape[0]), lag))
        return tu.blend_fit_cpu(cells, lag)
    for name, fn in (("frame_hist", frame_hist), ("frame_cells", frame_cells), ("hist_diff", hist_diff),
                     ("hist_diff_lag", hist_diff_lag), ("blend_fit", blend_fit)):
        monkeypatch.setattr(_lib, name, fn)
    return calls


def _kinds(calls):
    return [(c[0], int(c[1].shape[0]) if c[0] in ("hist", "cells") else c[1], *c[2:]) for c in calls]


def _uploads(calls):
    """the distinct slabs of frames that reached ``frame_hist`` or ``frame_cells``, in order"""
    seen = []
    for c in calls:
        if c[0] in ("hist", "cells") and not any(c[1] is s for s in seen):
            seen.append(c[1])
    return seen


def test_shot_transitions_in_any_grouping(spy):
    frames, (want, want_info) = _video()
    got, info = pred_func.shot_transitions(frames, dev="cpu")
    assert got == want == [(8, 13), (30, 34)] and tu.same_info(info, want_info)
    assert _kinds(spy) == [("hist", 38, 4, True), ("cells", 38, 16, True), ("fit", 38, 4), ("difflag", 38, 4), ("fit", 38, 8),
                           ("difflag", 38, 8)]
    spy.clear()
    small = pred_func.shot_transitions(frames, max_frames=4, dev="cpu")
    assert small[0] == want and tu.same_info(small[1], want_info)
    groups = [4] * 9 + [2]
    assert _kinds(spy)[:20] == [(k, n, g, True) for n in groups for k, g in (("hist", 4), ("cells", 16))]
    assert _kinds(spy)[20:] == [("fit", 38, 4), ("difflag", 38, 4), ("fit", 38, 8), ("difflag", 38, 8)]
    assert [int(s.shape[0]) for s in _uploads(spy)] == groups                  # every frame is uploaded once, for both
    tens = pred_func.shot_transitions(torch.as_tensor(frames), dev="cpu")
    assert tens[0] == want and tu.same_info(tens[1], want_info)
    # other grids, lags and thresholds reach the rule
    for kw in (dict(grid=32), dict(grid=8, regions=2), dict(lags=(3,)), dict(lags=[5, 4, 12]), dict(rho_max=0.2, h_min=0.0),
               dict(a_lo=0.3, a_hi=0.7, slack=0.0)):
        got, info = pred_func.shot_transitions(frames, dev="cpu", **kw)
        ref = tu.transitions_ref(frames, **kw)
        assert got == ref[0] and tu.same_info(info, ref[1]) and list(info) == list(kw.get("lags", (4, 8)))
    assert pred_func.shot_transitions(frames, rho_max=0.0, dev="cpu")[0] == []


def test_shot_transitions_of_few_frames_and_its_refusals(spy):
    import inspect
    frames, _ = _video()
    sig = inspect.signature(pred_func.shot_transitions).parameters              # one set of defaults, stated twice
    assert {k: sig[k].default for k in pred_func.TRANSITION_DEFAULTS} == pred_func.TRANSITION_DEFAULTS
    assert dict(pred_func.TRANSITION_DEFAULTS, regions=sig["regions"].default) == tu.DEFAULTS
    for few in (frames[:0], frames[:1], frames[:4], torch.as_tensor(frames[:3])):
        got, info = pred_func.shot_transitions(few, dev="cpu")
        assert got == [] and sorted(info) == [4, 8]
        for lag in (4, 8):
            assert info[lag]["a"].shape == info[lag]["rho"].shape == (0, lag - 1) and info[lag]["scores"].shape == (0,)
            assert info[lag]["scores"].dtype == np.float64 and info[lag]["blend"].dtype == bool
    assert spy == []                                                            # no lag below F: nothing is launched
    got, info = pred_func.shot_transitions(frames[:6], dev="cpu")               # lag 4 has two spans, lag 8 none
    assert info[4]["a"].shape == (2, 3) and info[8]["a"].shape == (0, 7)
    assert _kinds(spy) == [("hist", 6, 4, True), ("cells", 6, 16, True), ("fit", 6, 4), ("difflag", 6, 4)]
    spy.clear()
    for bad in (dict(lags=()), dict(lags=4), dict(lags=(2,)), dict(lags=(33,)), dict(lags=(4, 4)), dict(lags=(4.0,)),
                dict(lags=(True, 4)), dict(lags=None), dict(grid=4), dict(grid=64), dict(grid=16.0), dict(grid=True),
                dict(regions=3), dict(regions=16), dict(h_min=-0.1), dict(h_min=1.5), dict(h_min="0.2"), dict(rho_max=-1e-3),
                dict(rho_max=float("nan")), dict(a_lo=-0.1), dict(a_hi=1.1), dict(a_lo=0.6, a_hi=0.5), dict(a_lo=0.5, a_hi=0.5),
                dict(slack=-0.01), dict(slack=None), dict(max_frames=0)):
        with pytest.raises(ValueError):
            pred_func.shot_transitions(frames, dev="cpu", **bad)
    with pytest.raises(_lib.GenConViTHipError):
        pred_func.shot_transitions(frames.astype(np.float32), dev="cpu")
    with pytest.raises(_lib.GenConViTHipError):
        pred_func.shot_transitions(frames[..., :2], dev="cpu")
    assert spy == []


def test_the_bindings_refuse_host_tensors_and_bad_arguments_before_any_launch():
    """reaches no device: the checks come before the first call into the library's kernels"""
    frames = torch.as_tensor(cu.noise_video())
    for call in (lambda: _lib.frame_cells(frames), lambda: _lib.frame_cells(frames.numpy()),
                 lambda: _lib.blend_fit(torch.zeros((9, 256), dtype=torch.int32), 4),
                 lambda: _lib.hist_diff_lag(torch.zeros((9, 16, 64), dtype=torch.int32), 4)):
        with pytest.raises(_lib.GenConViTHipError):
            call()
    assert {"gcv_frame_cells", "gcv_blend_fit", "gcv_hist_diff_lag"} <= set(_lib.SIGNATURES)


# ----------------------------------------------------------------------------- scan_frames(transitions=...)
@pytest.fixture
def on_cpu(monkeypatch):
    monkeypatch.setattr(_lib, "face_crop_preprocess", su.face_crop_preprocess_ref)

    def vote_windows(logits, batch, nets, ranges):
        frame_p, mean2 = su.vote_windows_ref(logits, batch, nets, ranges)
        return frame_p.float(), mean2.float()
    monkeypatch.setattr(_lib, "vote_windows", vote_windows)


PLAIN_KEYS = ["boxes", "frame_scores", "segments", "track_offsets", "track_verdicts", "tracks", "verdict", "window_means",
              "windows"]


def _touches(first, last, transitions):
    return any(first <= b and a <= last for a, b in transitions)


def _same(a, b):
    return sorted(a) == sorted(b) and all(torch.equal(a[k], b[k]) if torch.is_tensor(a[k]) else
                                          np.array_equal(a[k], b[k]) if isinstance(a[k], np.ndarray) else a[k] == b[k] for k in a)


def test_scan_frames_without_transitions_is_unchanged(spy, on_cpu):
    frames, _ = _video()
    boxes = [(f, *cu.FACE_BOX) for f in range(38)]
    kw = dict(boxes=boxes, window=3, stride=1, max_batch=4)
    plain = pred_func.scan_frames(frames, StandIn(), **kw)
    assert sorted(plain) == PLAIN_KEYS and plain["tracks"] == [boxes] and spy == []
    assert _same(pred_func.scan_frames(frames, StandIn(), transitions=None, **kw), plain) and spy == []
    with_cuts = pred_func.scan_frames(frames, StandIn(), cuts=True, **kw)
    assert sorted(with_cuts) == sorted(PLAIN_KEYS + ["cuts", "cut_scores"])
    assert _kinds(spy) == [("hist", 4, 4, True)] * 9 + [("hist", 2, 4, True), ("diff", 38)]   # as before: no cells, no lags
    assert _same(pred_func.scan_frames(frames, StandIn(), cuts=True, transitions=None, transition_args=dict(grid=5), **kw),
                 with_cuts)


def test_scan_frames_keeps_the_frames_of_a_transition_out_of_tracks(spy, on_cpu):
    frames, _ = _video()
    boxes = [(f, *cu.FACE_BOX) for f in range(38)]
    kw = dict(boxes=boxes, window=3, stride=1, max_batch=4)
    plain = pred_func.scan_frames(frames, StandIn(), **kw)
    assert any(_touches(w[1], w[2], [(8, 13)]) for w in plain["windows"])       # what the option is for
    res = pred_func.scan_frames(frames, StandIn(), transitions=[(8, 13)], **kw)
    assert spy == [] and sorted(res) == sorted(PLAIN_KEYS + ["transitions"]) and res["transitions"] == [(8, 13)]
    assert res["tracks"] == [boxes[:8], boxes[14:]] and res["boxes"] == boxes[:8] + boxes[14:]
    assert res["tracks"][0][-1][0] == 7 and res["tracks"][1][0][0] == 14 and res["track_offsets"] == [0, 8, 32]
    assert not any(8 <= b[0] <= 13 for b in res["boxes"]) and res["frame_scores"].shape == (32, 2)
    assert res["windows"] and not any(_touches(w[1], w[2], [(8, 13)]) for w in res["windows"])
    assert not any(_touches(s[1], s[2], [(8, 13)]) for s in res["segments"])
    # the crops that remain are scored as they were
    keep = [f for f in range(38) if not 8 <= f <= 13]
    assert torch.equal(res["frame_scores"], plain["frame_scores"][keep])
    # a box that the detector saw on every second frame is not interpolated into or across the transition
    sparse = pred_func.scan_frames(frames, StandIn(), transitions=[(8, 13)], detect_every=2, window=3,
                                   boxes=[b for b in boxes if b[0] % 2 == 0])
    assert [[b[0] for b in t] for t in sparse["tracks"]] == [list(range(0, 7)), list(range(14, 37))]
    # with the hard cuts: they stay what ``cuts`` reports, the tracks end at both
    both = pred_func.scan_frames(frames, StandIn(), transitions=[(30, 34), (8, 13)], cuts=[22], **kw)
    assert both["transitions"] == [(8, 13), (30, 34)] and both["cuts"] == [22]
    assert [(t[0][0], t[-1][0]) for t in both["tracks"]] == [(0, 7), (14, 21), (22, 29), (35, 37)]
    # at the ends of the video: first = 0 and last + 1 = F make no cut, the boxes still go
    edge = pred_func.scan_frames(frames, StandIn(), transitions=[(0, 2), (36, 37)], **kw)
    assert [(t[0][0], t[-1][0]) for t in edge["tracks"]] == [(3, 35)]
    none = pred_func.scan_frames(frames, StandIn(), transitions=[], **kw)
    assert none["transitions"] == [] and none["tracks"] == [boxes]
    gone = pred_func.scan_frames(frames, StandIn(), transitions=[(0, 37)], **kw)
    assert gone["tracks"] == [] and gone["verdict"] == (None, None)


def test_scan_frames_measures_cuts_and_transitions_in_one_pass(spy, on_cpu):
    frames, (want, want_info) = _video()
    boxes = [(f, *cu.FACE_BOX) for f in range(38)]
    kw = dict(boxes=boxes, window=3, stride=1, max_batch=4)
    res = pred_func.scan_frames(frames, StandIn(), transitions=True, **kw)
    assert res["transitions"] == want and tu.same_info(res["transition_info"], want_info) and "cuts" not in res
    assert sorted(res) == sorted(PLAIN_KEYS + ["transitions", "transition_info"])
    assert [(t[0][0], t[-1][0]) for t in res["tracks"]] == [(0, 7), (14, 29), (35, 37)]
    assert [int(s.shape[0]) for s in _uploads(spy)] == [4] * 9 + [2]
    spy.clear()
    both = pred_func.scan_frames(frames, StandIn(), transitions=True, cuts=True, **kw)
    groups = [4] * 9 + [2]
    assert _kinds(spy)[:20] == [(k, n, g, True) for n in groups for k, g in (("hist", 4), ("cells", 16))]
    assert sorted(_kinds(spy)[20:]) == sorted([("fit", 38, 4), ("difflag", 38, 4), ("fit", 38, 8), ("difflag", 38, 8), ("diff", 38)])
    assert [int(s.shape[0]) for s in _uploads(spy)] == groups                  # one upload a group feeds both passes
    cuts, scores = pred_func.shot_cuts(frames, dev="cpu")
    assert both["cuts"] == cuts and (both["cut_scores"] == scores).all() and tu.HARD_CUT in cuts
    assert both["transitions"] == want and tu.same_info(both["transition_info"], want_info)
    ends = {t[-1][0] for t in both["tracks"]}
    starts = {t[0][0] for t in both["tracks"]}
    assert {7, 21, 29} <= ends and {14, 22} <= starts
    assert not any(_touches(b[0], b[0], want) for b in both["boxes"])
    assert not any(_touches(w[1], w[2], want) for w in both["windows"])
    # the arguments reach the rule
    loose = pred_func.scan_frames(frames, StandIn(), transitions=True, transition_args=dict(grid=32, lags=(4,)), **kw)
    ref = tu.transitions_ref(frames, grid=32, lags=(4,))
    assert loose["transitions"] == ref[0] and tu.same_info(loose["transition_info"], ref[1])
    # too few frames for any lag: nothing is measured, nothing is a transition
    spy.clear()
    short = pred_func.scan_frames(frames[:4], StandIn(), transitions=True, boxes=boxes[:4], window=3)
    assert short["transitions"] == [] and spy == [] and short["tracks"] == [boxes[:4]]


def test_scan_frames_refuses_bad_transitions_before_anything_runs(spy, on_cpu, monkeypatch):
    frames, _ = _video()
    kw = dict(boxes=[(f, *cu.FACE_BOX) for f in range(38)], window=3)
    monkeypatch.setattr(pred_func, "track_boxes", lambda *a, **k: pytest.fail("ran"))
    for bad in ([(8,)], [(8, 13, 2)], [8, 13], [(13, 8)], [(-1, 3)], [(30, 38)], [(8.0, 13)], [("8", 13)], [(True, 3)],
                [(None, 3)], "ab", False, 5, {(8, 13)}, np.array([[8, 13]])):
        with pytest.raises(ValueError):
            pred_func.scan_frames(frames, StandIn(), transitions=bad, **kw)
    for bad in (dict(lags=(2,)), dict(grid=5), dict(rho_max=-1.0), dict(regions=4), dict(threshold=0.1), [("grid", 16)]):
        with pytest.raises(ValueError):
            pred_func.scan_frames(frames, StandIn(), transitions=True, transition_args=bad, **kw)
    with pytest.raises(ValueError):
        pred_func.scan_frames(frames, StandIn(), transitions=True, cut_regions=3, **kw)
    assert spy == []
