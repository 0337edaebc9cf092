"""Carrying tracks past their first and last detection, without a GPU: the CPU restatement of ``gcv_track_chain``
(tests/extendutil.py) on a chain whose answer is known, and the host logic around it (``extend_tracks``,
``scan_frames(extend=True)``) with ``_lib.track_chain`` replaced by that restatement behind the binding's own row checks."""
import inspect
import os
import re

import numpy as np
import pytest
import torch

from genconvit_amd import _lib
from genconvit_amd.model import pred_func
from tests import extendutil as eu
from tests import followutil as fu
from tests import personutil as pu
from tests import scanutil as su

torch.set_grad_enabled(False)
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEVER = eu.STOP_NEVER


# ----------------------------------------------------------------------------- the restatement
def _stepping_video():
    """4 grey frames of 64 x 80 (R = G = B, so the luma is the value): a 32 x 32 patch whose 2 x 2 pixel blocks each have one
    value of their own, 20 + 13 i + j for block row i and column j, on a background of 0, at (top, left) = (10, 20), then moved
    by (+4, +2), (-2, +6) and (0, -4) pixels — whole cells of the 16-grid of a 32 x 32 box (a cell is 2 x 2 pixels)"""
    i, j = np.mgrid[0:32, 0:32] // 2
    patch = (20 + 13 * i + j).astype(np.uint8)
    frames = np.zeros((4, 64, 80, 3), dtype=np.uint8)
    at = [(10, 20), (14, 22), (12, 28), (12, 24)]
    for f, (t, l) in enumerate(at):
        frames[f, t:t + 32, l:l + 32] = patch[..., None]
    return frames, patch, at


def test_a_hand_worked_three_step_chain():
    frames, patch, at = _stepping_video()
    cells = patch[::2, ::2].astype(np.int64)                                 # the template's cells: one per block
    job = (0, 10, 52, 42, 20, 1, 1, 3, 0, 0, NEVER)
    out = eu.track_chain_ref(frames, [job], 16, 4)
    assert out.dtype == np.int32 and out.shape == (1, 3, 4)
    # the patch is found exactly (cost 0: every cell is one block), each step relative to the step before
    assert out[0, :, :3].tolist() == [[4, 2, 0], [-2, 6, 0], [0, -4, 0]]
    # cost0, by hand: the window at the prior is the patch shifted by the step's (dy, dx) = (oy, ox) / 2 cells, 0 outside
    for k, (dy, dx) in enumerate([(2, 1), (-1, 3), (0, -2)]):
        moved = np.zeros((16, 16), dtype=np.int64)
        ys, xs = slice(max(dy, 0), 16 + min(dy, 0)), slice(max(dx, 0), 16 + min(dx, 0))
        moved[ys, xs] = cells[max(-dy, 0):16 - max(dy, 0), max(-dx, 0):16 - max(dx, 0)]
        assert int(out[0, k, 3]) == int(np.abs(cells - moved).sum())
    # backward from frame 3 the same path in reverse; a stop below the cost of not moving changes nothing (the best is 0)
    back = eu.track_chain_ref(frames, [(3, 12, 56, 44, 24, 2, -1, 3, 0, 0, 0)], 16, 4)
    assert back[0, :, :3].tolist() == [[0, 4, 0], [2, -6, 0], [-4, -2, 0]]
    # radius 1 cannot reach (2, 1): it takes the best it can see, and stop = that cost - 1 ends the chain there
    near = eu.track_chain_ref(frames, [job], 16, 1)
    assert near[0, 0, 2] > 0 and max(abs(int(near[0, 0, 0])), abs(int(near[0, 0, 1]))) <= 2
    cut = eu.track_chain_ref(frames, [(*job[:10], int(near[0, 0, 2]) - 1)], 16, 1)
    assert cut[0].tolist() == [list(eu.NONE)] * 3
    # continued from the first step's offset: the rest of the chain; rows past ``steps`` hold the refusal row
    rest = eu.track_chain_ref(frames, [(0, 10, 52, 42, 20, 2, 1, 2, 4, 2, NEVER)], 16, 4, max_steps=3)
    assert rest[0].tolist() == out[0, 1:].tolist() + [list(eu.NONE)]


def test_the_two_writings_of_the_restatement_agree():
    for case in (eu.moving_case, eu.stop_case, eu.border_case):
        frames, jobs, grid, radius = case()
        assert np.array_equal(eu.track_chain_alt(frames, jobs, grid, radius), eu.track_chain_ref(frames, jobs, grid, radius))
    frames, jobs = eu.random_case(16)
    assert np.array_equal(eu.track_chain_alt(frames, jobs, 16, 5), eu.track_chain_ref(frames, jobs, 16, 5))


def test_the_default_cost_max_is_midway_on_the_synthetic_material():
    follows, gone = eu.policy_costs(radius=pred_func.EXTEND_DEFAULTS["radius"])
    print(f"\nlargest cost per cell of a step that follows {follows:.3f}, smallest after the pattern is gone {gone:.3f}")
    assert round(follows, 1) == 9.8 and round(gone, 1) == 27.6
    assert pred_func.EXTEND_DEFAULTS["cost_max"] == round((follows + gone) / 2, 1) == 18.7
    for text in (pred_func.extend_tracks.__doc__, open(os.path.join(REPO, "DESIGN.md")).read()):
        assert "9.8" in text and "27.6" in text and "18.7" in text


def test_the_defaults_are_stated_once():
    seen = set()
    for f in (pred_func.extend_tracks, pred_func._check_extend):
        sig = inspect.signature(f).parameters
        assert all(sig[k].default == v for k, v in pred_func.EXTEND_DEFAULTS.items()), f
        seen |= set(sig) & set(pred_func.EXTEND_DEFAULTS)
    assert seen == set(pred_func.EXTEND_DEFAULTS) == {"grid", "radius", "steps", "cost_max"}
    src = inspect.getsource(pred_func)
    assert len(re.findall(r"cost_max=\d", src)) == 1 and len(re.findall(r"steps=\d", src)) == 1      # the dict itself
    assert "extend_args" in inspect.signature(pred_func.scan_frames).parameters


# ----------------------------------------------------------------------------- extend_tracks
@pytest.fixture
def spy(monkeypatch):
    """``_lib.track_chain`` is the restatement behind the binding's own row checks; every call is recorded as (frames of
    the slab, job rows, grid, radius)"""
    calls = []

    def track_chain(frames_u8, jobs, grid=64, radius=8):
        jobs = [tuple(int(v) for v in j) for j in jobs]
        calls.append((frames_u8.shape[0], jobs, grid, radius))
        _lib._check_chain_jobs("track_chain", jobs, *frames_u8.shape[:3], grid)
        return torch.as_tensor(eu.track_chain_ref(frames_u8, jobs, grid, radius))
    monkeypatch.setattr(_lib, "track_chain", track_chain)
    return calls


def _box(f):
    t, l = eu.MOVE_PATH[f]
    return (f, t, l + eu.MOVE_W, t + eu.MOVE_H, l)


ARGS = dict(grid=16, radius=5, cost_max=40.0)


def _walk(box, d, steps):
    out = []
    for oy, ox, _, _ in steps:
        box = (box[0] + d, box[1] + oy, box[2] + ox, box[3] + oy, box[4] + ox)
        out.append(box)
    return out


def test_extend_tracks_builds_one_chain_each_way_and_adds_the_boxes(spy):
    frames, _, grid, radius = eu.moving_case()
    stop = int(40.0 * 256)
    tracks = [[_box(2), _box(3)]]
    got, ext = pred_func.extend_tracks(frames, tracks, steps=8, dev="cpu", **ARGS)
    assert spy == [(6, [(*_box(2), 1, -1, 2, 0, 0, stop)], 16, 5), (4, [(1, *_box(3)[1:], 2, 1, 2, 0, 0, stop)], 16, 5)] or \
        len(spy) == 1                                                          # grouping is checked below; here: the rows
    rows = [r for c in spy for r in c[1]]
    assert sorted((r[6], r[7]) for r in rows) == [(-1, 2), (1, 2)] and all(r[8:] == (0, 0, stop) for r in rows)
    fwd = eu.track_chain_ref(frames, [(*_box(3), 4, 1, 2, 0, 0, stop)], 16, 5)[0]
    bwd = eu.track_chain_ref(frames, [(*_box(2), 1, -1, 2, 0, 0, stop)], 16, 5)[0]
    assert got == [_walk(_box(2), -1, bwd.tolist())[::-1] + tracks[0] + _walk(_box(3), 1, fwd.tolist())]
    assert [b[0] for b in got[0]] == list(range(6)) and tracks == [[_box(2), _box(3)]]      # the input is not changed
    assert ext.dtype == np.int32 and ext[:, :3].tolist() == [[0, 4, 1], [0, 5, 1], [0, 1, -1], [0, 0, -1]]
    assert ext[:2, 3:].tolist() == fwd.tolist() and ext[2:, 3:].tolist() == bwd.tolist()
    # on the path: within a cell (3 x 2.5 pixels) of the truth
    assert all(abs(b[1] - eu.MOVE_PATH[b[0]][0]) <= 3 and abs(b[4] - eu.MOVE_PATH[b[0]][1]) <= 3 for b in got[0])


def test_extend_tracks_stops_at_steps_at_the_video_borders_and_at_ends(spy):
    frames, _, _, _ = eu.moving_case()
    frames_of = lambda **kw: [b[0] for b in pred_func.extend_tracks(frames, [[_box(2)]], dev="cpu", **{**ARGS, **kw})[0][0]]
    assert frames_of(steps=8) == [0, 1, 2, 3, 4, 5]                          # the video's borders
    assert frames_of(steps=1) == [1, 2, 3] and frames_of(steps=2) == [0, 1, 2, 3, 4]
    assert frames_of(steps=8, ends=[4]) == [0, 1, 2, 3]                     # a new shot starts at 4
    assert frames_of(steps=8, ends=[1, 5]) == [1, 2, 3, 4]                  # backward: the shot's first frame is taken
    assert frames_of(steps=8, ends=[2, 3]) == [2]                           # a shot of one frame
    assert frames_of(steps=8, ends=[3, 2, 2]) == [2]                        # any order, any repeats
    assert frames_of(steps=8, ends=[]) == frames_of(steps=8, ends=None) == [0, 1, 2, 3, 4, 5]
    at_end = pred_func.extend_tracks(frames, [[_box(0)], [_box(5)]], steps=1, iou=1.1, dev="cpu", **ARGS)[0]
    assert [[b[0] for b in tr] for tr in at_end] == [[0, 1], [4, 5]]         # nothing before frame 0 or after frame 5


def test_extend_tracks_stops_at_the_cost_bound(spy):
    frames, jobs, grid, radius = eu.stop_case()
    box = jobs[0][:5]
    costs = eu.track_chain_ref(frames, [jobs[0]], grid, radius)[0, :, 2]
    cell = lambda c: c / 256.0
    run = lambda cost_max: pred_func.extend_tracks(frames, [[box]], grid=16, radius=4, steps=8, cost_max=cost_max, dev="cpu")
    got, ext = run(cell(costs[2]) - 1e-6)                                   # floor(...) = costs[2] - 1: frame 3 is refused
    assert [b[0] for b in got[0]] == [0, 1, 2] and ext[:, 5].tolist() == costs[:2].tolist()
    got, ext = run(cell(costs[2]))                                          # the bound itself passes
    assert [b[0] for b in got[0]] == [0, 1, 2, 3, 4, 5]
    assert [b[0] for b in run(0.0)[0][0]] == [0] and run(0.0)[1].shape == (0, 7)
    assert all(c[1][0][10] == s for c, s in zip(spy, (int(costs[2]) - 1, int(costs[2]), 0, 0)))


def test_extend_tracks_gives_small_boxes_no_chain(spy):
    frames, _, _, _ = eu.moving_case()
    got, ext = pred_func.extend_tracks(frames, [[_box(2)]], grid=64, radius=5, steps=4, cost_max=40.0, dev="cpu")   # 48 x 40 < 64
    assert got == [[_box(2)]] and ext.shape == (0, 7) and ext.dtype == np.int32 and spy == []
    narrow = (2, 20, 45, 60, 30)                                            # 40 x 15
    tracks = [[narrow, _box(3)]]                                            # backward from the narrow box: none; forward: yes
    got, ext = pred_func.extend_tracks(frames, tracks, steps=4, dev="cpu", **ARGS)
    assert got[0][:2] == tracks[0] and (ext[:, 2] == 1).all() and len(ext) == 2


def test_the_collision_rule_in_both_orders(spy):
    """a face that a detector drop-out split in two: track 0 ends in frame 1, track 1 starts in frame 4, on the moving pattern.
    The forward chain of track 0 is taken first and runs up to frame 3 — in frame 4 it meets track 1's own box; track 1's
    backward chain then finds frame 3 taken by track 0's extension.  With the tracks in the other order the forward
    chains still go first, so the same track owns the gap."""
    frames, _, _, _ = eu.moving_case()
    a, b = [_box(0), _box(1)], [_box(4), _box(5)]
    got, ext = pred_func.extend_tracks(frames, [a, b], steps=8, dev="cpu", **ARGS)
    assert [[x[0] for x in tr] for tr in got] == [[0, 1, 2, 3], [4, 5]]
    assert ext[:, :3].tolist() == [[0, 2, 1], [0, 3, 1]]
    got, ext = pred_func.extend_tracks(frames, [b, a], steps=8, dev="cpu", **ARGS)
    assert [[x[0] for x in tr] for tr in got] == [[4, 5], [0, 1, 2, 3]]
    assert ext[:, :3].tolist() == [[1, 2, 1], [1, 3, 1]]
    # backward chains among themselves, and forward ones: track order decides
    got, ext = pred_func.extend_tracks(frames, [[_box(5)], [_box(4)]], steps=1, dev="cpu", **ARGS)
    assert [[x[0] for x in tr] for tr in got] == [[5], [3, 4]]              # 5 -> 4 meets track 1's box; 4 -> 5 meets track 0's
    # an IoU bound nothing reaches: every chain runs its length, and the face is covered twice
    got, ext = pred_func.extend_tracks(frames, [a, b], steps=8, iou=1.1, dev="cpu", **ARGS)
    assert [[x[0] for x in tr] for tr in got] == [[0, 1, 2, 3, 4, 5], [0, 1, 2, 3, 4, 5]]
    # two faces that are apart do not stop each other
    far = [(0, 60, 125, 92, 90)]
    got, _ = pred_func.extend_tracks(frames, [[_box(2)], far], steps=8, dev="cpu", **ARGS)
    assert [x[0] for x in got[0]] == [0, 1, 2, 3, 4, 5]


def test_extend_tracks_groups_host_frames_and_continues_a_chain(spy):
    frames, _, _, _ = eu.moving_case()
    tracks = [[_box(0)]]
    whole, ext = pred_func.extend_tracks(frames, tracks, steps=8, dev="cpu", **ARGS)
    assert [c[0] for c in spy] == [6] and spy[0][1][0][5:8] == (1, 1, 5)
    del spy[:]
    parts, ext4 = pred_func.extend_tracks(frames, tracks, steps=8, max_frames=4, dev="cpu", **ARGS)
    assert parts == whole and (ext4 == ext).all()                            # the continued chain equals the undivided one
    assert [c[0] for c in spy] == [4, 3]                                    # frames {0, 1, 2, 3}, then {0, 4, 5}
    first, second = spy[0][1][0], spy[1][1][0]
    assert first[:5] == _box(0) and first[5:10] == (1, 1, 3, 0, 0)
    assert second[0] == 0 and second[1:5] == _box(0)[1:] and second[5:8] == (1, 1, 2)      # remapped: 4 -> 1
    assert second[8:10] == (int(ext[:3, 3].sum()), int(ext[:3, 4].sum()))
    del spy[:]
    parts, ext2 = pred_func.extend_tracks(frames, tracks, steps=8, max_frames=2, dev="cpu", **ARGS)
    assert parts == whole and (ext2 == ext).all() and [c[0] for c in spy] == [2] * 5
    # two tracks, both ways, in groups of 4: the same boxes as in one launch
    del spy[:]
    both = [[_box(2)], [(3, 60, 125, 92, 90)]]
    one = pred_func.extend_tracks(frames, both, steps=8, dev="cpu", **ARGS)
    n = len(spy)
    many = pred_func.extend_tracks(frames, both, steps=8, max_frames=4, dev="cpu", **ARGS)
    assert n == 1 and len(spy) > 2 and all(c[0] <= 4 for c in spy[1:]) and many[0] == one[0] and (many[1] == one[1]).all()
    # a chain that stopped is not continued
    del spy[:]
    frames, jobs, grid, radius = eu.stop_case()
    c = eu.track_chain_ref(frames, [jobs[0]], grid, radius)[0, :, 2]
    got, _ = pred_func.extend_tracks(frames, [[jobs[0][:5]]], grid=16, radius=4, steps=8, cost_max=(int(c[2]) - 1) / 256.0 + 1e-9,
                                     max_frames=3, dev="cpu")
    assert [b[0] for b in got[0]] == [0, 1, 2] and len(spy) == 2             # {0, 1, 2}, {0, 3, 4} stops at once, {0, 5} is not sent


def test_extend_tracks_on_nothing_and_its_refusals(spy):
    frames, _, _, _ = eu.moving_case()
    got, ext = pred_func.extend_tracks(frames, [], dev="cpu")
    assert got == [] and ext.shape == (0, 7) and ext.dtype == np.int32 and spy == []
    tracks = [[_box(2)]]
    for bad in (dict(grid=48), dict(grid=16.0), dict(radius=-1), dict(radius=33), dict(steps=0), dict(steps=1025),
                dict(steps=2.5), dict(steps=True), dict(cost_max=-1), dict(cost_max=256), dict(cost_max="low"),
                dict(cost_max=None), dict(max_frames=1)):
        with pytest.raises(ValueError):
            pred_func.extend_tracks(frames, tracks, **{**ARGS, **bad})
    with pytest.raises(_lib.GenConViTHipError):
        pred_func.extend_tracks(frames.astype(np.float32), tracks, **ARGS)
    with pytest.raises(_lib.GenConViTHipError):
        pred_func.extend_tracks(frames, [[(2, 20, 129, 60, 80)]], **ARGS)
    assert spy == []


# ----------------------------------------------------------------------------- scan_frames(extend=True)
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
    from tests import qualityutil as qu
    seen = {"quality": [], "sig": []}
    monkeypatch.setattr(_lib, "face_crop_preprocess", lambda frames_u8, boxes, size=224, dtype=None:
                        su.face_crop_preprocess_ref(frames_u8, boxes, size, dtype))

    def vote_windows(logits, batch, nets, ranges):
        frame_p, mean2 = su.vote_windows_ref(logits, batch, nets, ranges)
        return frame_p.float(), mean2.float()

    def face_quality(frames_u8, boxes, grid=64):
        seen["quality"].append(len(boxes))
        return torch.as_tensor(qu.face_quality_ref(frames_u8, [tuple(int(v) for v in b) for b in boxes], grid))

    def face_signature(frames_u8, boxes):
        seen["sig"].append(len(boxes))
        return torch.as_tensor(pu.face_signature_ref(frames_u8, [tuple(int(v) for v in b) for b in boxes]))
    monkeypatch.setattr(_lib, "vote_windows", vote_windows)
    monkeypatch.setattr(_lib, "face_quality", face_quality)
    monkeypatch.setattr(_lib, "face_signature", face_signature)
    monkeypatch.setattr(_lib, "sig_link", lambda sig, owner, tracks: torch.as_tensor(
        pu.sig_link_ref(sig, np.asarray(owner), tracks)))
    return seen


PLAIN_KEYS = ["boxes", "frame_scores", "segments", "track_offsets", "track_verdicts", "tracks", "verdict", "window_means",
              "windows"]
SCAN = dict(detect_every=4, window=3, extend_args=dict(grid=16, radius=4, steps=8, cost_max=40.0))


def _interview_seen_once_a_shot():
    """tests/personutil.py's interview (16 frames, cuts at 4, 8, 12), the detector's boxes on frames 1, 5, 9, 13 only"""
    frames, det, cuts = pu.interview()
    return frames, [d for d in det if d[0] % 4 == 1], cuts


def test_scan_frames_scores_the_frames_up_to_the_cut_and_none_past_it(spy, on_cpu):
    frames, det, cuts = _interview_seen_once_a_shot()
    plain = pred_func.scan_frames(frames, StandIn(), boxes=det, cuts=cuts, detect_every=4, window=3)
    assert sorted(plain) == sorted(PLAIN_KEYS + ["cuts"]) and [len(t) for t in plain["tracks"]] == [1, 1, 1, 1] and spy == []
    res = pred_func.scan_frames(frames, StandIn(), boxes=det, cuts=cuts, extend=True, **SCAN)
    assert sorted(res) == sorted(PLAIN_KEYS + ["cuts", "extend"])
    # every shot: one frame back to the cut, two forward to the frame before the next cut; 8 steps were allowed
    assert [[b[0] for b in tr] for tr in res["tracks"]] == [[0, 1, 2, 3], [4, 5, 6, 7], [8, 9, 10, 11], [12, 13, 14, 15]]
    assert len(res["boxes"]) == 16 and res["track_offsets"] == [0, 4, 8, 12, 16] and tuple(res["frame_scores"].shape) == (16, 2)
    assert res["extend"].shape == (12, 7) and res["extend"][:, :3].tolist() == \
        [[t, 4 * t + k, 1] for t in range(4) for k in (2, 3)] + [[t, 4 * t, -1] for t in range(4)]
    assert all(res["tracks"][t][1] == det[t] for t in range(4))
    assert all(abs(b[1] - d[1]) <= 3 and abs(b[4] - d[4]) <= 3 for tr, d in zip(res["tracks"], det) for b in tr)
    # the crops are those of the extended boxes
    want = su.vote_windows_ref(StandIn()(su.face_crop_preprocess_ref(frames, res["boxes"])), 16, 1, [])[0]
    assert (res["frame_scores"].double() - want).abs().max().item() <= 1e-6
    # no chain was given a frame past a cut: every job stays inside its shot
    for _, jobs, _, _ in spy:
        for j in jobs:
            assert {(j[5] + j[6] * k) // 4 for k in range(j[7])} == {j[0] // 4}
    # without the cuts only the cost gate stands at a cut: a generous one lets the chains walk into the next shots (iou = 1.1:
    # no collision), a strict one stops them there — the cuts are what keeps the frames past a cut unscored above
    loose = pred_func.scan_frames(frames, StandIn(), boxes=det, extend=True, iou=1.1, **SCAN)
    assert [b[0] for b in loose["tracks"][0]] == list(range(10)) and [b[0] for b in loose["tracks"][3]] == list(range(5, 16))
    cost = {(int(r[0]), int(r[1])): r[5] / 256.0 for r in loose["extend"]}
    print(f"\ncost per cell inside the shot {max(cost[0, 2], cost[0, 3]):.1f}, across the cut {cost[0, 4]:.1f}")
    strict = pred_func.scan_frames(frames, StandIn(), boxes=det, extend=True, iou=1.1,
                                   **{**SCAN, "extend_args": dict(grid=16, radius=4, steps=8, cost_max=(cost[0, 3] + cost[0, 4]) / 2)})
    assert [b[0] for b in strict["tracks"][0]] == [0, 1, 2, 3]
    # eps counts the crops after extension
    with pytest.raises(ValueError, match="16 crops"):
        pred_func.scan_frames(frames, StandIn(), boxes=det, cuts=cuts, extend=True, eps=torch.zeros(4, 8), **SCAN)


def test_quality_and_persons_see_the_extended_rows(spy, on_cpu):
    frames, det, cuts = _interview_seen_once_a_shot()
    _, top, right, bottom, left = det[1]
    frames[6, top - 3:bottom + 3, left - 3:right + 3] = 0                    # an extended frame of shot 1, painted black
    res = pred_func.scan_frames(frames, StandIn(), boxes=det, cuts=cuts, extend=True, quality=True,
                                quality_args=dict(grid=16), persons=True, **SCAN)
    assert sorted(res) == sorted(PLAIN_KEYS + ["cuts", "extend", "quality", "persons"])
    q = res["quality"]
    assert on_cpu["quality"] == [len(q["boxes"])] and len(q["boxes"]) >= 13 and [b[0] for b in q["boxes"]][:6] == [0, 1, 2, 3, 4, 5]
    # the chain of shot 1 stops at the black frame by its cost, so the gate is shown a frame that was measured and kept
    assert 6 not in [b[0] for b in q["boxes"]] and [b[0] for b in res["tracks"][1]] == [4, 5]
    assert sum(on_cpu["sig"]) == len(res["boxes"]) == len(res["persons"]["rows"]) and len(res["boxes"]) > len(det)
    assert res["persons"]["tracks"] == [[0, 2], [1, 3]]


def test_scan_frames_without_extend_is_unchanged_and_refuses_bad_arguments(spy, on_cpu, monkeypatch):
    frames, det, cuts = _interview_seen_once_a_shot()
    kw = dict(boxes=det, cuts=cuts, detect_every=4, window=3)
    base = pred_func.scan_frames(frames, StandIn(), **kw)
    for more in (dict(extend=None), dict(extend=None, extend_args=dict(nonsense=1))):
        res = pred_func.scan_frames(frames, StandIn(), **kw, **more)
        assert sorted(res) == sorted(PLAIN_KEYS + ["cuts"])
        for key in res:
            assert torch.equal(res[key], base[key]) if torch.is_tensor(res[key]) else res[key] == base[key]
    assert spy == []
    none = pred_func.scan_frames(frames, StandIn(), boxes=[], extend=True)
    assert none["verdict"] == (None, None) and none["extend"].shape == (0, 7) and spy == []
    monkeypatch.setattr(pred_func, "track_boxes", lambda *a, **k: pytest.fail("ran"))
    for bad in (dict(extend=False), dict(extend=1), dict(extend="yes"), dict(extend_args=dict(grid=20)),
                dict(extend_args=dict(radius=33)), dict(extend_args=dict(steps=0)), dict(extend_args=dict(cost_max=-0.5)),
                dict(extend_args=dict(iou=0.5)), dict(extend_args=[("grid", 16)]), dict(extend_args=dict(cost_max="high"))):
        with pytest.raises(ValueError):
            pred_func.scan_frames(frames, StandIn(), **kw, **{"extend": True, **bad})
    assert spy == []


# ----------------------------------------------------------------------------- the binding's refusals
def test_the_binding_rejects_bad_rows_before_any_launch(monkeypatch):
    monkeypatch.setattr(_lib, "check", lambda *a, **k: pytest.fail("launched"))
    ok = (0, 20, 60, 68, 20, 1, 1, 2, 0, 0, 100)
    check = lambda row, grid=16: _lib._check_chain_jobs("t", [row], 3, 96, 128, grid)
    assert tuple(check(ok).shape) == (1, 11) and tuple(_lib._check_chain_jobs("t", [], 3, 96, 128, 16).shape) == (0, 11)
    edit = lambda **kw: tuple(kw.get(f"c{i}", v) for i, v in enumerate(ok))
    bad = [edit(c0=3), edit(c0=-1), edit(c5=3), edit(c5=-1), edit(c7=3), edit(c5=0, c6=-1, c7=2),   # frame indices
           edit(c3=97), edit(c2=129), edit(c1=-1), edit(c4=-2),                                  # the template box
           edit(c8=-21), edit(c8=29), edit(c9=-21), edit(c9=69),                                 # the first prior box
           edit(c3=35), edit(c2=35),                                                             # a side below the grid
           edit(c6=0), edit(c6=2), edit(c7=0), edit(c7=1025), edit(c10=-1)]
    for row in bad:
        with pytest.raises(_lib.GenConViTHipError):
            check(row)
    with pytest.raises(_lib.GenConViTHipError):
        check(ok, grid=64)
    check(edit(c8=-20, c9=68))
    check(edit(c8=28, c9=-20))
    check(edit(c5=2, c6=-1, c7=3, c10=2 ** 31 - 1))
    frames = torch.zeros((3, 96, 128, 3), dtype=torch.uint8)
    with pytest.raises(_lib.GenConViTHipError, match="device tensor"):
        _lib.track_chain(frames, [ok], grid=16, radius=4)


def test_the_header_declares_the_entry_and_states_its_arithmetic():
    hdr = open(os.path.join(REPO, "include", "genconvit_hip.h")).read()
    assert re.search(r"int gcv_track_chain\(const void\* frames_u8_nhwc, int nframes, int H, int W, const int\* jobs11, int n, "
                     r"int max_steps, int grid,\s+int radius, int\* out4, gcv_stream s\);", hdr)
    assert len(_lib.SIGNATURES["gcv_track_chain"][1]) == 11
    for word in ("fa, top, right, bottom, left", "fs, dir, steps", "py, px", "(0, 0, -1, -1)", "cost > stop",
                 "(frame, prior box, template, 1, template, 0)", "tests/extendutil.py"):
        assert word in hdr, word
    assert "Extending a track past\n * its first and last detection is gcv_track_chain's" in hdr
    assert "``extend_tracks``" in pred_func.follow_tracks.__doc__ and "``extend``" in pred_func.scan_frames.__doc__
