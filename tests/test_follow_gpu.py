"""``gcv_track_match`` on the MI355X, bit for bit against its CPU restatement (tests/followutil.py: all four columns,
``torch.equal``, no tolerance — the arithmetic is integer), its refusals, and ``pred_func.scan_frames(follow=True)`` end to
end with synthetic weights."""
import numpy as np
import pytest
import torch

from genconvit_amd import _lib, synth
from genconvit_amd.model import pred_func
from genconvit_amd.model.genconvit import GenConViT
from tests import followutil as fu

pytestmark = pytest.mark.gpu
torch.set_grad_enabled(False)

_CACHE = {}


def _cached(key, make):
    if key not in _CACHE:
        _CACHE[key] = make()
    return _CACHE[key]


def _assert_same(frames, jobs, grid, radius):
    dev = _cached(("dev", id(frames)), lambda: torch.as_tensor(frames).cuda())
    got = _lib.track_match(dev, jobs, grid=grid, radius=radius)
    assert got.is_cuda and got.dtype == torch.int32 and tuple(got.shape) == (len(jobs), 4)
    want = torch.as_tensor(fu.track_match_ref(frames, jobs, grid, radius))
    if not torch.equal(got.cpu(), want):
        bad = (got.cpu() != want).any(1).nonzero().flatten().tolist()
        raise AssertionError(f"grid {grid} radius {radius}: jobs {bad} differ; first: job {jobs[bad[0]]} got "
                             f"{got[bad[0]].tolist()} want {want[bad[0]].tolist()}")
    return got


def test_track_match_path_case():
    frames, jobs, priors = _cached("path", fu.path_case)
    got = _assert_same(frames, jobs, 16, 4).cpu()
    assert [(p[0] + int(o[0]), p[1] + int(o[1])) for p, o in zip(priors, got)] == fu.PATH_FOLLOWED
    assert int(got[1, 2]) == 0 and bool((got[:, 2] < got[:, 3]).all())


@pytest.mark.parametrize("radius", [0, 1, 5, 8])
@pytest.mark.parametrize("grid", [16, 32])
def test_track_match_random_jobs(grid, radius):
    """3 x 120 x 160 frames, two of noise and a smooth one; 48 jobs with sides that are no multiple of the grid, three
    different sizes per job, weights with wa = 0 and wb = 0, priors on all four borders.  No two candidates of a job share
    its smallest cost (tests/test_follow_sensitivity_cpu.py asserts it): the key's tie-break is decided by the tie cases
    below, not here."""
    frames, jobs = _cached(("fuzz", grid), lambda: fu.fuzz_case(lo=grid))
    sides = [(j[c + 3] - j[c + 1], j[c + 2] - j[c + 4]) for j in jobs for c in (0, 5, 11)]
    assert all(grid <= s <= 100 and s % 16 for hw in sides for s in hw)
    assert any(j[10] == 0 for j in jobs) and any(j[16] == 0 for j in jobs)
    assert {0} == {min(j[1] for j in jobs), min(j[4] for j in jobs)} and max(j[3] for j in jobs) == 120 and \
        max(j[2] for j in jobs) == 160
    got = _assert_same(frames, jobs, grid, radius).cpu()
    if radius == 0:
        assert bool((got[:, :2] == 0).all()) and torch.equal(got[:, 2], got[:, 3])


@pytest.mark.parametrize("radius", [32, 16])
def test_track_match_largest_configuration(radius):
    """grid 64 with radius 32: the largest LDS footprint and the most candidates; 3 x 256 x 256 frames, boxes of 64 ... 120"""
    frames, jobs = _cached("large", fu.largest_case)
    _assert_same(frames, jobs, 64, radius)


@pytest.mark.parametrize("grid,k,radius", fu.TIE_CASES)
def test_track_match_ties_are_broken_by_d2_then_dy_then_dx(grid, k, radius):
    """two identical frames that are constant along the anti-diagonals: job A costs 0 on all of dy + dx = +1, job B on all of
    dy + dx = -2, and the rows are what d2, then dy, then dx pick — at radius 8 among 289 candidates, so the equal costs sit
    in different waves and in both trips of the candidate loop"""
    frames, jobs = _cached(("tie", grid, k), lambda: fu.tie_case(grid, k))
    got = _assert_same(frames, jobs, grid, radius).cpu()
    assert got.tolist() == fu.TIE_ROWS[(grid, k, radius)]


@pytest.mark.parametrize("up,left", [(8, 7), (6, 6)])
@pytest.mark.parametrize("grid,k", [(16, 3), (32, 2)])
def test_track_match_best_in_the_second_trip_and_the_fourth_wave(grid, k, up, left):
    """the tie frames with the prior far off, radius 8: (8, 7) leaves cost 0 to candidates 271 and 287 alone, both in the
    second trip of the 256-lane loop; (6, 6) gives the row to candidate 252, in the fourth wave"""
    frames, jobs = _cached(("far tie", grid, k, up, left), lambda: fu.far_tie_case(grid, k, up, left))
    got = _assert_same(frames, jobs, grid, 8).cpu()
    want = [7 * k, 8 * k, 0] if (up, left) == (8, 7) else [6 * k, 6 * k, 0]
    assert got[0, :3].tolist() == want


def test_track_match_at_the_cost_bound():
    """grid 64, black templates on a white window, wa + wb = 1024: cost = 1024 * 4096 * 255 = 1 069 547 520, the kernel's
    stated bound; every candidate costs that, so the answer is (0, 0)"""
    frames, jobs, grid, radius = _cached("bound", fu.bound_case)
    got = _assert_same(frames, jobs, grid, radius).cpu()
    assert got.tolist() == [[0, 0, fu.COST_BOUND, fu.COST_BOUND]] * 3 and fu.COST_BOUND == 1069547520


def test_track_match_refusals_and_no_jobs():
    frames, jobs, _ = _cached("path", fu.path_case)
    dev = torch.as_tensor(frames).cuda()
    none = _lib.track_match(dev, [], grid=16, radius=4)
    assert tuple(none.shape) == (0, 4) and none.dtype == torch.int32 and none.is_cuda
    for kw in (dict(grid=8), dict(grid=48), dict(grid=128), dict(radius=-1), dict(radius=33)):
        with pytest.raises(_lib.GenConViTHipError):
            _lib.track_match(dev, jobs, **{"grid": 16, "radius": 4, **kw})
    with pytest.raises(_lib.GenConViTHipError):
        _lib.track_match(dev, jobs, grid=64, radius=4)                        # 48 x 40 boxes on a grid of 64
    with pytest.raises(_lib.GenConViTHipError):
        _lib.track_match(dev, [(5, *jobs[0][1:])], grid=16, radius=4)         # frame 5 of 5
    with pytest.raises(_lib.GenConViTHipError):
        _lib.track_match(dev, [(*jobs[0][:10], 0, *jobs[0][11:16], 0)], grid=16, radius=4)
    with pytest.raises(_lib.GenConViTHipError):
        _lib.track_match(dev.cpu(), jobs, grid=16, radius=4)                  # a host tensor never reaches a launch
    # the launcher's own checks, through the C ABI: bad scalars are refused with a reason and nothing is launched
    lib = _lib.load()
    jd = torch.as_tensor(jobs, dtype=torch.int32).cuda()
    out = torch.full((3, 4), -7, dtype=torch.int32, device="cuda")
    stream = _lib.current_stream_ptr(dev.device)
    call = lambda nf=5, h=96, w=128, n=3, grid=16, radius=4: lib.gcv_track_match(dev.data_ptr(), nf, h, w, jd.data_ptr(), n,
                                                                                grid, radius, out.data_ptr(), stream)
    for kw in (dict(grid=8), dict(grid=0), dict(grid=65), dict(radius=-1), dict(radius=33), dict(nf=0), dict(h=0),
               dict(w=-1)):
        assert call(**kw) != 0 and _lib.last_error()
        with pytest.raises(_lib.GenConViTHipError):
            _lib.check(call(**kw), "gcv_track_match")
    assert call(n=0) == 0
    torch.cuda.synchronize()
    assert bool((out == -7).all())                                            # nothing was launched so far
    # rows the binding would refuse give zeros and read nothing; the valid row beside them is served
    rows = [jobs[0], (9, *jobs[1][1:]), (*jobs[2][:3], 400, *jobs[2][4:])]
    jd.copy_(torch.as_tensor(rows, dtype=torch.int32))
    assert call() == 0
    want = fu.track_match_ref(frames, jobs[:1], 16, 4)
    assert out.cpu().tolist() == [want[0].tolist(), [0, 0, 0, 0], [0, 0, 0, 0]]
    # and a valid call after all that is correct
    _assert_same(frames, jobs, 16, 4)


# ----------------------------------------------------------------------------- scan_frames(follow=True) end to end
def _ensemble():
    """the fp16 ensemble of tests/test_scan_gpu.py: the same cached networks, built once per session"""
    from tests.test_scan_gpu import _ed, _vae
    return GenConViT.from_modules(_ed(torch.float16), _vae(torch.float16), net="genconvit")


def test_scan_frames_follow_on_the_device():
    """9 frames, the detector on every fourth; a face on a curve and a static one.  The followed boxes are the
    restatement's, the static face does not move, and the scores are those of a scan that is given the followed boxes as
    per-frame detections: the same crops through the same launches."""
    frames, det, path = fu.two_face_video()
    model = _ensemble()
    eps = synth.make_eps(18, name="follow").cuda()
    kw = dict(iou=0.05, window=4, stride=2, eps=eps)
    res = pred_func.scan_frames(frames, model, boxes=det, detect_every=4, follow=True, follow_grid=16, follow_radius=4, **kw)
    # the restatement of the whole host path: interpolate, match on the CPU, move
    tracks, anchors = pred_func.track_boxes(det, iou=0.05, max_gap=4, return_anchors=True)
    assert [len(t) for t in tracks] == [9, 9] and anchors[0] == [f % 4 == 0 for f in range(9)]
    jobs, where = [], []
    for t, tr in enumerate(tracks):
        for f in (1, 2, 3, 5, 6, 7):
            fa, fb = f // 4 * 4, f // 4 * 4 + 4
            jobs.append((*tr[f], *tr[fa], fb - f, *tr[fb], f - fa))
            where.append((t, f))
    want = fu.track_match_ref(frames, jobs, 16, 4)
    moved = [list(tr) for tr in tracks]
    for (t, f), (oy, ox, _, _) in zip(where, want.tolist()):
        b = moved[t][f]
        moved[t][f] = (f, b[1] + oy, b[2] + ox, b[3] + oy, b[4] + ox)
    assert res["tracks"] == moved and res["boxes"] == moved[0] + moved[1]
    assert res["follow"].dtype == np.int32 and res["follow"][:, :2].tolist() == [list(w) for w in where]
    assert (res["follow"][:, 2:] == want).all()
    assert (res["follow"][6:, 2:4] == 0).all() and moved[1] == tracks[1]                   # the static face
    off = [abs(b[1] - p[0]) + abs(b[4] - p[1]) for b, p in zip(moved[0], path)]
    lin = [abs(b[1] - p[0]) + abs(b[4] - p[1]) for b, p in zip(tracks[0], path)]
    print(f"\nfollow: |box - truth| per frame, interpolated {lin}, followed {off}")
    assert all(o <= l for o, l in zip(off, lin)) and sum(off) < sum(lin)       # nowhere further off, in sum closer
    # the same crops, the same launches
    again = pred_func.scan_frames(frames, model, boxes=res["boxes"], detect_every=1, **kw)
    assert again["tracks"] == res["tracks"] and "follow" not in again
    assert torch.equal(again["frame_scores"], res["frame_scores"])
    assert torch.equal(again["window_means"], res["window_means"]) and again["windows"] == res["windows"]
    # device frames take the in-place path: one launch, the same answer
    dev = pred_func.scan_frames(torch.as_tensor(frames).cuda(), model, boxes=det, detect_every=4, follow=True,
                                follow_grid=16, follow_radius=4, **kw)
    assert dev["tracks"] == res["tracks"] and (dev["follow"] == res["follow"]).all()
    assert torch.equal(dev["frame_scores"], res["frame_scores"])
