"""Keeping blurred and badly exposed faces out of the votes, without a GPU: the CPU restatement of ``gcv_face_quality``
(tests/qualityutil.py) on cases whose answers are known, what blur does to it, and the host logic around it
(``quality_keep``, ``face_quality``, ``scan_frames(quality=True)``) with ``_lib.face_quality`` replaced by that restatement."""
import inspect
import os
import re

import numpy as np
import pytest
import torch

from genconvit_amd import _lib
from genconvit_amd.model import pred_func
from tests import followutil as fu
from tests import qualityutil as qu
from tests import scanutil as su

torch.set_grad_enabled(False)
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _one(img, grid):
    """the row of the whole image as one box"""
    h, w = img.shape[:2]
    return qu.face_quality_ref(img[None], [(0, 0, w, h, 0)], grid)[0].tolist()


# ----------------------------------------------------------------------------- the restatement: known answers
@pytest.mark.parametrize("grid", [16, 32, 64])
def test_flat_black_and_white_boxes(grid):
    n = grid * grid
    img = qu.flat(70, 90, 0)
    img[:] = (10, 200, 30)                                   # Y = (770 + 30000 + 870 + 128) >> 8 = 124
    assert _one(img, grid) == [grid, n * 124, n * 124 * 124, 0, 0, 0, 0, 0]
    assert _one(qu.flat(70, 90, 0), grid) == [grid, 0, 0, 0, 0, 0, n, 0]
    assert _one(qu.flat(70, 90, 255), grid) == [grid, n * 255, n * 255 * 255, 0, 0, 0, 0, n]
    assert _one(qu.flat(70, 90, 15), grid)[6:] == [n, 0] and _one(qu.flat(70, 90, 16), grid)[6:] == [0, 0]
    assert _one(qu.flat(70, 90, 239), grid)[6:] == [0, 0] and _one(qu.flat(70, 90, 240), grid)[6:] == [0, n]


@pytest.mark.parametrize("grid", [16, 32])
def test_a_single_bright_cell(grid):
    """a box of 2G x 2G pixels, cells of 2 x 2, value a everywhere but a + d in one cell.  The Laplacian is 4 d at that cell
    and -d at each of its four neighbours, and only interior cells (u, v in [1, G - 1)) count:
      well inside (the cell and its four neighbours interior)   L2 = (4 d)^2 + 4 d^2 = 20 d^2
      at u = 1 (the neighbour above lies in row 0)              L2 = 16 d^2 + 3 d^2
      at (1, 1)                                                  L2 = 16 d^2 + 2 d^2
      at u = 0, v inside (the cell is not interior; only the neighbour below is)   L2 = d^2
      in the corner (0, 0)                                       L2 = 0
    A cell with both row neighbours gives GX = 2 d^2, one at the left or right border d^2; GY alike."""
    a, d, n = 40, 100, grid * grid
    for (u, v), l2, gx, gy in (((5, 7), 20, 2, 2), ((1, 7), 19, 2, 2), ((1, 1), 18, 2, 2), ((0, 7), 1, 2, 1),
                               ((0, 0), 0, 1, 1), ((grid - 1, grid - 2), 1, 2, 1), ((grid - 2, grid - 2), 18, 2, 2)):
        img = qu.flat(2 * grid, 2 * grid, a)
        img[2 * u:2 * u + 2, 2 * v:2 * v + 2] = a + d
        assert _one(img, grid) == [grid, n * a + d, (n - 1) * a * a + (a + d) ** 2, l2 * d * d, gx * d * d, gy * d * d, 0, 0]


@pytest.mark.parametrize("grid", [16, 32, 64])
def test_the_cells_of_a_box_one_pixel_over_the_grid_tile_it(grid):
    """G x (G + 1) pixels: e(v) = v (G + 1) // G = v for v < G and G + 1 for v = G — every cell is one pixel but those of the
    last column, which hold two and take their rounded mean"""
    rng = np.random.default_rng(4)
    Y = rng.integers(0, 256, (grid + 9, grid + 11)).astype(np.int64)
    c, ey, ex = qu.cells_ref(Y, (3, 5 + grid + 1, 3 + grid, 5), grid)
    assert ey.tolist() == list(range(grid + 1)) and ex.tolist() == list(range(grid)) + [grid + 1]
    box = Y[3:3 + grid, 5:5 + grid + 1]
    assert (c[:, :grid - 1] == box[:, :grid - 1]).all()
    assert (c[:, grid - 1] == (box[:, grid - 1] + box[:, grid] + 1) // 2).all()
    c, ey, ex = qu.cells_ref(Y, (3, 5 + grid, 3 + grid + 1, 5), grid)                      # (G + 1) x G: the same down the rows
    assert ey.tolist() == list(range(grid)) + [grid + 1] and ex.tolist() == list(range(grid + 1))
    for extent in range(grid, 4 * grid):                                                   # strictly rising from 0 to the extent
        e = [fu.edge(u, extent, grid) for u in range(grid + 1)]
        assert e[0] == 0 and e[-1] == extent and all(x < y for x, y in zip(e, e[1:]))


def test_the_stated_bounds_hold_at_their_worst():
    """a checkerboard of 0 and 255 cells makes every Laplacian +-1020 and every difference +-255"""
    for grid in (16, 32, 64):
        u, v = np.mgrid[0:grid, 0:grid]
        row = qu.quality_of_cells(255 * ((u + v) % 2))
        assert row[3] == (grid - 2) ** 2 * 1020 ** 2 and row[4] == row[5] == grid * (grid - 1) * 255 ** 2
        assert row[2] == grid * grid // 2 * 255 ** 2
    assert 62 ** 2 * 1020 ** 2 > 2 ** 31 and 16 * 1020 ** 2 < 2 ** 24 and 64 * 16 * 1020 ** 2 < 2 ** 31


# ----------------------------------------------------------------------------- the restatement: what blur does
@pytest.mark.parametrize("grid,sides", [(64, (64, 100, 150, 200)), (32, (32, 64, 100, 150))])
def test_an_isotropic_blur_lowers_the_sharpness(grid, sides):
    for side in sides:
        sharp = qu.texture(side, side + 3, seed=5)
        a = qu.measures(_one(sharp, grid))[0][0]
        b = qu.measures(_one(qu.box_blur(sharp, 9, 9), grid))[0][0]
        print(f"\ngrid {grid} side {side}: sharpness {a:.1f} -> {b:.1f}, {a / b:.1f}-fold")
        assert a >= 4.0 * b


def test_the_grid_must_follow_the_face_size():
    """the figures the docstring of ``pred_func.face_quality`` quotes: a 200-pixel face, 9-pixel blur"""
    sharp = qu.texture(200, 203, seed=5)
    soft = qu.box_blur(sharp, 9, 9)
    fold = {g: qu.measures(_one(sharp, g))[0][0] / qu.measures(_one(soft, g))[0][0] for g in (16, 64)}
    assert 25.0 <= fold[64] <= 35.0 and 1.5 <= fold[16] <= 2.5, fold


@pytest.mark.parametrize("grid,side", [(64, 200), (64, 100), (32, 100)])
def test_a_horizontal_blur_lowers_gx_against_gy(grid, side):
    sharp = qu.texture(side, side + 3, seed=5)
    _, gx, gy = qu.measures(_one(sharp, grid))
    _, mx, my = qu.measures(_one(qu.box_blur(sharp, 1, 15), grid))
    print(f"\ngrid {grid} side {side}: gx / gy {gx[0] / gy[0]:.2f} -> {mx[0] / my[0]:.2f}")
    assert 0.8 <= gx[0] / gy[0] <= 1.25 and mx[0] / my[0] < 0.5
    _, vx, vy = qu.measures(_one(qu.box_blur(sharp, 15, 1), grid))                        # and a vertical one the other way
    assert vy[0] / vx[0] < 0.5


# ----------------------------------------------------------------------------- quality_keep
def _quality(sharp, dark=None, bright=None, measured=None):
    n = len(sharp)
    m = np.ones(n, dtype=bool) if measured is None else np.asarray(measured, dtype=bool)
    val = lambda v: np.where(m, np.asarray(v if v is not None else np.zeros(n), dtype=np.float64), np.nan)
    return {"measured": m, "sharpness": val(sharp), "dark": val(dark), "bright": val(bright)}


def test_quality_keep_median_rule_is_per_track():
    q = _quality([100, 100, 40, 100, 60, 10, 10, 10, 4, 10])
    keep = pred_func.quality_keep(q, [0, 5, 10])
    assert keep.dtype == bool and keep.tolist() == [True, True, False, True, True, True, True, True, False, True]
    assert pred_func.quality_keep(q, [0, 10]).tolist() == [True, True, True, True, True] + [False] * 5    # one track: median 25
    assert pred_func.quality_keep(q, [0, 5, 10], sharp_rel=0.0).all()
    assert pred_func.quality_keep(q, [0, 5, 10], sharp_rel=0.0, sharp_min=50).tolist() == [True, True, False, True, True] + \
        [False] * 5
    assert pred_func.quality_keep(q, [0, 5, 10], sharp_rel=0.7).tolist() == [True, True, False, True, False, True, True, True,
                                                                            False, True]
    assert pred_func.quality_keep(q, [0, 0, 5, 5, 10]).tolist() == keep.tolist()             # empty tracks
    assert pred_func.quality_keep(_quality([]), [0]).shape == (0,)
    assert pred_func.quality_keep(_quality([0, 0, 0]), [0, 3]).all()                         # a flat track: 0 < 0 is false


def test_quality_keep_keeps_unmeasured_rows():
    q = _quality([100, 1, 100, 1, 100], measured=[True, False, True, True, False], dark=[0, 1, 0, 0, 1])
    assert pred_func.quality_keep(q, [0, 5]).tolist() == [True, True, True, False, True]     # the median is over the measured
    q = _quality([1, 2, 3], measured=[False] * 3)
    assert pred_func.quality_keep(q, [0, 3], sharp_min=1000).all()


def test_quality_keep_clip_rule():
    q = _quality([50] * 6, dark=[0, 0.5, 0.51, 0, 0, 1], bright=[0, 0, 0, 0.5, 0.75, 0])
    assert pred_func.quality_keep(q, [0, 6]).tolist() == [True, True, False, True, False, False]
    assert pred_func.quality_keep(q, [0, 6], clip_max=1.0).all()
    assert pred_func.quality_keep(q, [0, 6], clip_max=0.25).tolist() == [True, False, False, False, False, False]


def test_quality_keep_refuses_bad_parameters():
    q = _quality([1, 2, 3])
    for bad in (dict(sharp_rel=-0.1), dict(sharp_rel=1.1), dict(sharp_min=-1), dict(clip_max=0), dict(clip_max=1.5),
                dict(clip_max=-0.5), dict(sharp_rel=float("nan")), dict(sharp_min=True)):
        with pytest.raises(ValueError):
            pred_func.quality_keep(q, [0, 3], **bad)
    for offs in ([0, 2], [1, 3], [0, 2, 1, 3], []):
        with pytest.raises(ValueError):
            pred_func.quality_keep(q, offs)
    pred_func.quality_keep(q, [0, 3], sharp_rel=1.0, sharp_min=0, clip_max=1)


def test_the_defaults_are_stated_once():
    for f in (pred_func.quality_keep, pred_func.face_quality, pred_func._check_quality):
        sig = inspect.signature(f).parameters
        assert [k for k in pred_func.QUALITY_DEFAULTS if k in sig], f
        assert all(sig[k].default == v for k, v in pred_func.QUALITY_DEFAULTS.items() if k in sig), f


# ----------------------------------------------------------------------------- face_quality
@pytest.fixture
def spy(monkeypatch):
    """``_lib.face_quality`` is the restatement behind the binding's own row checks; every call is recorded as (frames of
    the slab, rows, grid)"""
    calls = []

    def face_quality(frames_u8, boxes, grid=64):
        boxes = [tuple(int(v) for v in b) for b in boxes]
        calls.append((frames_u8.shape[0], boxes, grid))
        _lib._check_quality_boxes("face_quality", boxes, *frames_u8.shape[:3], grid)
        return torch.as_tensor(qu.face_quality_ref(frames_u8, boxes, grid))
    monkeypatch.setattr(_lib, "face_quality", face_quality)
    return calls


def _scattered():
    """5 frames of 60 x 80 noise and 7 boxes, out of frame order, two of them too small for a grid of 16"""
    frames = np.random.default_rng(12).integers(0, 256, (5, 60, 80, 3), dtype=np.uint8)
    boxes = [(4, 0, 80, 60, 0), (0, 5, 40, 30, 10), (2, 10, 25, 40, 10), (4, 20, 50, 50, 10), (1, 1, 30, 16, 3),
             (0, 30, 80, 60, 40), (2, 0, 17, 16, 0)]
    return frames, boxes, [0, 1, 3, 5, 6]                    # box 2 is 15 wide, box 4 15 high; box 6 is 16 x 17


def test_face_quality_measures_in_the_order_of_the_boxes(spy):
    frames, boxes, big = _scattered()
    q = pred_func.face_quality(frames, boxes, grid=16)
    assert sorted(q) == sorted(["raw", "measured", "sharpness", "gx", "gy", "mean", "contrast", "dark", "bright"])
    assert q["measured"].tolist() == [i in big for i in range(7)] and q["measured"].dtype == bool
    want = qu.face_quality_ref(frames, [boxes[i] for i in big], 16)
    assert q["raw"].dtype == np.int64 and (q["raw"][big] == want).all() and (q["raw"][[2, 4]] == 0).all()
    s, gx, gy = qu.measures(want)
    for key, val in (("sharpness", s), ("gx", gx), ("gy", gy), ("mean", want[:, 1] / 256.0),
                     ("contrast", want[:, 2] / 256.0 - (want[:, 1] / 256.0) ** 2), ("dark", want[:, 6] / 256.0),
                     ("bright", want[:, 7] / 256.0)):
        assert q[key].dtype == np.float64 and np.array_equal(q[key][big], val), key
        assert np.isnan(q[key][[2, 4]]).all(), key
    # one group: the three frames that carry a measured box (0, 2, 4), in frame order, the rows remapped into the slab
    assert len(spy) == 1 and spy[0][0] == 3 and spy[0][2] == 16
    assert spy[0][1] == [(0, *boxes[1][1:]), (0, *boxes[5][1:]), (1, *boxes[6][1:]), (2, *boxes[0][1:]), (2, *boxes[3][1:])]


@pytest.mark.parametrize("max_frames,slabs", [(1, [1, 1, 1]), (2, [2, 1]), (128, [3])])
def test_face_quality_groups_by_the_frames_a_group_needs(spy, max_frames, slabs):
    frames, boxes, big = _scattered()
    one = pred_func.face_quality(frames, boxes, grid=16)
    del spy[:]
    q = pred_func.face_quality(frames, boxes, grid=16, max_frames=max_frames)
    assert [c[0] for c in spy] == slabs                                                    # frames 0, 2, 4 carry the boxes
    assert sum(len(c[1]) for c in spy) == len(big) and all(r[0] < c[0] for c in spy for r in c[1])
    assert all(np.array_equal(q[k], one[k], equal_nan=True) for k in one)
    dev = pred_func.face_quality(torch.as_tensor(frames), boxes, grid=16, max_frames=max_frames)      # a host tensor alike
    assert all(np.array_equal(dev[k], one[k], equal_nan=True) for k in one)


def test_face_quality_without_boxes_and_with_bad_arguments(spy):
    frames, boxes, _ = _scattered()
    q = pred_func.face_quality(frames, [], grid=16)
    assert q["raw"].shape == (0, 8) and q["measured"].shape == (0,) and q["sharpness"].shape == (0,) and spy == []
    q = pred_func.face_quality(frames, [boxes[2], boxes[4]], grid=16)                       # nothing large enough: no launch
    assert not q["measured"].any() and spy == []
    assert not pred_func.face_quality(frames, boxes[:2], grid=64)["measured"].any() and spy == []
    for bad in (dict(grid=8), dict(grid=48), dict(grid=True), dict(max_frames=0)):
        with pytest.raises(ValueError):
            pred_func.face_quality(frames, boxes, **{"grid": 16, **bad})
    with pytest.raises(_lib.GenConViTHipError):
        pred_func.face_quality(frames, [(0, 0, 81, 60, 0)], grid=16)
    with pytest.raises(_lib.GenConViTHipError):
        pred_func.face_quality(frames.astype(np.float32), boxes, grid=16)
    assert spy == []


# ----------------------------------------------------------------------------- scan_frames(quality=True)
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
    crops = []

    def face_crop_preprocess(frames_u8, boxes, size=224, dtype=None):
        crops.append(len(boxes))
        return su.face_crop_preprocess_ref(frames_u8, boxes, size, dtype)
    monkeypatch.setattr(_lib, "face_crop_preprocess", face_crop_preprocess)

    def vote_windows(logits, batch, nets, ranges):
        frame_p, mean2 = su.vote_windows_ref(logits, batch, nets, ranges)
        return frame_p.float(), mean2.float()
    monkeypatch.setattr(_lib, "vote_windows", vote_windows)
    return crops


PLAIN_KEYS = ["boxes", "frame_scores", "segments", "track_offsets", "track_verdicts", "tracks", "verdict", "window_means",
              "windows"]
QARGS = dict(grid=16)                                        # the faces are 48 x 40 and 40 x 40 pixels


def test_scan_frames_without_quality_is_unchanged(spy, on_cpu):
    frames, det = qu.gated_video()
    for kw in ({}, dict(quality=None), dict(quality=False), dict(quality=None, quality_args=dict(nonsense=1))):
        res = pred_func.scan_frames(frames, StandIn(), boxes=det, window=3, **kw)
        assert sorted(res) == PLAIN_KEYS and len(res["boxes"]) == 20
    assert spy == []


def test_scan_frames_drops_the_planted_rows_before_it_crops(spy, on_cpu):
    frames, det = qu.gated_video()
    plain = pred_func.scan_frames(frames, StandIn(), boxes=det, window=3)
    del on_cpu[:]
    res = pred_func.scan_frames(frames, StandIn(), boxes=det, window=3, quality=True, quality_args=QARGS)
    assert sorted(res) == sorted(PLAIN_KEYS + ["quality"])
    q = res["quality"]
    assert q["boxes"] == plain["boxes"] and len(q["boxes"]) == 20                           # the rows before the gate
    assert (q["raw"] == qu.face_quality_ref(frames, plain["boxes"], 16)).all() and q["measured"].all()
    planted = [i for i, b in enumerate(q["boxes"]) if b[1:] == qu.FACE_A and b[0] in qu.PLANTED]
    assert planted == [4, 5, 6] and np.nonzero(~q["kept"])[0].tolist() == planted
    assert q["track_map"] == [0, 1]
    # the tracks, the rows and everything after them describe what is left
    a = [(f, *qu.FACE_A) for f in range(10) if f not in qu.PLANTED]
    assert res["tracks"] == [a, plain["tracks"][1]] and res["boxes"] == a + plain["tracks"][1]
    assert res["track_offsets"] == [0, 7, 17] and tuple(res["frame_scores"].shape) == (17, 2)
    assert sum(on_cpu) == 17                                                               # 17 crops were cut, not 20
    kept_rows = [i for i in range(20) if i not in planted]
    assert torch.equal(res["frame_scores"], plain["frame_scores"][kept_rows])              # the same crops, the same scores
    # no window (and so no segment) covers a crop of a planted frame: a window is a run of the kept rows
    assert [w[:3] for w in res["windows"]] == [(t, tr[lo][0], tr[hi - 1][0]) for t, tr in enumerate(res["tracks"])
                                               for lo, hi in pred_func.window_ranges(len(tr), 3, 1)]
    fp = res["frame_scores"].double()
    for k, (t, first, last, _, _) in enumerate(res["windows"]):
        rows = [res["track_offsets"][t] + i for i, b in enumerate(res["tracks"][t]) if first <= b[0] <= last]
        assert len(rows) == 3 and all(res["boxes"][r][0] not in qu.PLANTED or t == 1 for r in rows)
        assert (res["window_means"][k].double() - fp[rows].mean(0)).abs().max().item() <= 1e-6
    for seg in res["segments"]:
        assert any(w[0] == seg[0] and w[1] == seg[1] and w[3] == 0 for w in res["windows"])
    # eps counts the crops that remain
    ok = pred_func.scan_frames(frames, StandIn(), boxes=det, window=3, quality=True, quality_args=QARGS, eps=torch.zeros(17, 4))
    assert torch.equal(ok["frame_scores"], res["frame_scores"])
    with pytest.raises(ValueError, match="17 crops"):
        pred_func.scan_frames(frames, StandIn(), boxes=det, window=3, quality=True, quality_args=QARGS, eps=torch.zeros(20, 4))
    # the thresholds reach quality_keep
    none = pred_func.scan_frames(frames, StandIn(), boxes=det, window=3, quality=True, quality_args=dict(grid=16, sharp_rel=0.0))
    assert none["quality"]["kept"].all() and none["boxes"] == plain["boxes"]
    # max_batch is the group size of the quality pass too: host frames go up in slabs of at most two
    del spy[:]
    two = pred_func.scan_frames(frames, StandIn(), boxes=det, window=3, max_batch=2, quality=True, quality_args=QARGS)
    assert [c[0] for c in spy] == [2] * 5 and (two["quality"]["raw"] == q["raw"]).all() and two["boxes"] == res["boxes"]


def test_scan_frames_removes_a_track_that_loses_every_row(spy, on_cpu):
    frames, det = qu.gated_video(black_b=True)
    res = pred_func.scan_frames(frames, StandIn(), boxes=det, window=3, quality=True, quality_args=QARGS)
    q = res["quality"]
    assert (q["dark"][10:] == 1.0).all() and not q["kept"][10:].any() and q["kept"][:10].tolist() == [f not in qu.PLANTED
                                                                                                     for f in range(10)]
    assert q["track_map"] == [0] and len(res["tracks"]) == 1 and res["track_offsets"] == [0, 7]
    assert len(res["track_verdicts"]) == 1 and {w[0] for w in res["windows"]} == {0}
    # only the black face: every track goes, and nothing is cropped or voted
    del on_cpu[:]
    gone = pred_func.scan_frames(frames, StandIn(), boxes=det[1::2], window=3, quality=True, quality_args=QARGS)
    assert gone["verdict"] == (None, None) and gone["tracks"] == [] and gone["quality"]["track_map"] == [] and on_cpu == []
    assert len(gone["quality"]["boxes"]) == 10 and tuple(gone["frame_scores"].shape) == (0, 2)


def test_scan_frames_quality_without_a_face(spy, on_cpu):
    frames, _ = qu.gated_video()
    res = pred_func.scan_frames(frames, StandIn(), boxes=[], quality=True)
    assert res["verdict"] == (None, None) and spy == [] and on_cpu == []
    q = res["quality"]
    assert q["raw"].shape == (0, 8) and q["kept"].shape == (0,) and q["boxes"] == [] and q["track_map"] == []


def test_scan_frames_follows_before_it_measures(spy, on_cpu, monkeypatch):
    """the detector on every fourth frame of followutil's path case: the boxes that are measured are the followed ones"""
    order = []

    def track_match(frames_u8, jobs, grid=64, radius=16):
        order.append("follow")
        return torch.as_tensor(fu.track_match_ref(frames_u8, [tuple(int(v) for v in j) for j in jobs], grid, radius))
    monkeypatch.setattr(_lib, "track_match", track_match)
    measure = _lib.face_quality
    monkeypatch.setattr(_lib, "face_quality", lambda *a, **k: (order.append("quality"), measure(*a, **k))[1])
    frames, jobs, _ = fu.path_case()
    det = [jobs[0][5:10], jobs[0][11:16]]
    res = pred_func.scan_frames(frames, StandIn(), boxes=det, detect_every=4, iou=0.05, window=3, follow=True, follow_grid=16,
                                follow_radius=4, quality=True, quality_args=dict(grid=16, sharp_rel=0.0))
    assert order == ["follow", "quality"]
    assert [(b[1], b[4]) for b in res["quality"]["boxes"]] == [fu.PATH_TOPLEFT[0]] + fu.PATH_FOLLOWED + [fu.PATH_TOPLEFT[4]]
    assert spy[0][1] == res["quality"]["boxes"] and res["follow"].shape == (3, 6)
    assert (res["quality"]["raw"] == qu.face_quality_ref(frames, res["quality"]["boxes"], 16)).all()


def test_scan_frames_refuses_bad_quality_arguments_before_anything_runs(spy, on_cpu, monkeypatch):
    frames, det = qu.gated_video()
    monkeypatch.setattr(pred_func, "track_boxes", lambda *a, **k: pytest.fail("ran"))
    for bad in (dict(quality_args=dict(grid=8)), dict(quality_args=dict(grid=16, radius=3)), dict(quality_args=[("grid", 16)]),
                dict(quality_args=dict(sharp_rel=1.5)), dict(quality_args=dict(sharp_min=-1.0)),
                dict(quality_args=dict(clip_max=0.0)), dict(quality_args=dict(max_frames=4)), dict(quality="yes"),
                dict(quality=1)):
        with pytest.raises(ValueError):
            pred_func.scan_frames(frames, StandIn(), boxes=det, **{"quality": True, **bad})
    assert spy == [] and on_cpu == []


# ----------------------------------------------------------------------------- the binding's refusals
def test_the_binding_refuses_before_any_launch(monkeypatch):
    """none of these reaches the library: a launch without a GPU would fail differently"""
    monkeypatch.setattr(_lib, "check", lambda *a, **k: pytest.fail("launched"))
    frames = torch.zeros((2, 60, 80, 3), dtype=torch.uint8)
    with pytest.raises(_lib.GenConViTHipError, match="device tensor"):
        _lib.face_quality(frames, [(0, 0, 40, 40, 0)], grid=16)                            # a host tensor
    for grid in (8, 48, 128):
        with pytest.raises(_lib.GenConViTHipError, match="grid"):
            _lib.face_quality(frames, [(0, 0, 40, 40, 0)], grid=grid)
    check = lambda box, grid=16: _lib._check_quality_boxes("t", [box], 2, 60, 80, grid)
    assert tuple(check((1, 0, 80, 60, 0)).shape) == (1, 5) and tuple(_lib._check_quality_boxes("t", [], 2, 60, 80, 16).shape) == (0, 5)
    for box in ((2, 0, 40, 40, 0), (-1, 0, 40, 40, 0), (0, 0, 81, 40, 0), (0, 0, 40, 61, 0), (0, -1, 40, 40, 0),
                (0, 0, 40, 40, -1)):
        with pytest.raises(_lib.GenConViTHipError, match="outside"):
            check(box)
    for box in ((0, 0, 15, 40, 0), (0, 10, 40, 25, 0)):
        with pytest.raises(_lib.GenConViTHipError, match="smaller than grid"):
            check(box)
    check((0, 0, 16, 16, 0))
    with pytest.raises(_lib.GenConViTHipError, match="smaller than grid"):
        check((0, 0, 40, 40, 0), grid=64)


def test_the_header_declares_the_entry_and_states_its_arithmetic():
    hdr = open(os.path.join(REPO, "include", "genconvit_hip.h")).read()
    assert re.search(r"int gcv_face_quality\(const void\* frames_u8_nhwc, int nframes, int H, int W, const int\* boxes5, int n, "
                     r"int grid,\s+int64_t\* out8, gcv_stream stream\);", hdr)
    assert "gcv_face_quality" in _lib.SIGNATURES and len(_lib.SIGNATURES["gcv_face_quality"][1]) == 9
    for word in ("(G, S1, S2, L2, GX, GY, dark, bright)", "c < 16", "c > 239", "tests/qualityutil.py"):
        assert word in hdr, word
