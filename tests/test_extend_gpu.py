"""``gcv_track_chain`` on the MI355X, bit for bit against its CPU restatement (tests/extendutil.py: a loop over the
restatement of ``gcv_track_match``; all four columns of every step, ``torch.equal``, no tolerance — the arithmetic is
integer), against ``gcv_track_match`` itself on one-step chains, its refusals, and ``pred_func.scan_frames(extend=True)``
end to end with synthetic weights."""
import numpy as np
import pytest
import torch

from genconvit_amd import _lib, synth
from genconvit_amd.model import pred_func
from genconvit_amd.model.genconvit import GenConViT
from tests import extendutil as eu
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
    got = _lib.track_chain(dev, jobs, grid=grid, radius=radius)
    steps = max(j[7] for j in jobs)
    assert got.is_cuda and got.dtype == torch.int32 and tuple(got.shape) == (len(jobs), steps, 4)
    want = torch.as_tensor(eu.track_chain_ref(frames, jobs, grid, radius))
    if not torch.equal(got.cpu(), want):
        bad = (got.cpu() != want).flatten(1).any(1).nonzero().flatten().tolist()
        raise AssertionError(f"grid {grid} radius {radius}: jobs {bad} differ; first: job {jobs[bad[0]]} got "
                             f"{got[bad[0]].tolist()} want {want[bad[0]].tolist()}")
    return got.cpu()


def test_track_chain_follows_a_moving_pattern_forward_and_backward():
    """5 steps each way, a different displacement at every step, from the left border to the right and back"""
    frames, jobs, grid, radius = _cached("moving", eu.moving_case)
    got = _assert_same(frames, jobs, grid, radius)
    assert len({tuple(s[:2]) for s in got[0].tolist()}) == 5 and len({tuple(s[:2]) for s in got[1].tolist()}) == 5
    for job, rows, path in ((jobs[0], got[0], eu.MOVE_PATH[1:]), (jobs[1], got[1], eu.MOVE_PATH[4::-1])):
        t, l = job[1], job[4]
        for (oy, ox, cost, cost0), (tt, tl) in zip(rows.tolist(), path):
            t, l = t + oy, l + ox
            assert abs(t - tt) <= 3 and abs(l - tl) <= 3 and 0 <= cost < cost0      # a cell is 3 x 2.5 pixels


@pytest.mark.parametrize("radius", [0, 1, 5, 8])
@pytest.mark.parametrize("grid", [16, 32])
def test_track_chain_random_chains(grid, radius):
    """6 x 120 x 160 frames (noise, a flat one, a smooth one); 48 chains of 1 ... 5 steps in one launch, both directions,
    first priors off the template, templates on all four borders, and stops that end some chains"""
    frames, jobs = _cached(("random", grid), lambda: eu.random_case(grid))
    assert {j[7] for j in jobs} == {1, 2, 3, 4, 5} and {j[6] for j in jobs} == {1, -1}
    assert {0} == {min(j[1] for j in jobs), min(j[4] for j in jobs)} and max(j[3] for j in jobs) == 120 and \
        max(j[2] for j in jobs) == 160
    got = _assert_same(frames, jobs, grid, radius)
    if radius == 0:
        assert bool((got[..., :2] == 0).all()) and torch.equal(got[..., 2], got[..., 3])
    if grid == 32:
        ended = [bool((g[:j[7], 2] < 0).any()) for j, g in zip(jobs, got)]
        assert any(ended) and not all(ended)


def test_track_chain_stops_in_its_middle():
    frames, jobs, grid, radius = _cached("stop", eu.stop_case)
    got = _assert_same(frames, jobs, grid, radius)
    none = list(eu.NONE)
    assert (got[0, :, 2] >= 0).all() and got[1, :2].tolist() == got[0, :2].tolist() and got[1, 2:].tolist() == [none] * 3
    assert got[2].tolist() == got[1].tolist() and got[3].tolist() == got[0].tolist()      # stop = cost: goes on
    assert got[4].tolist() == [none] * 5 and got[5].tolist() == [none] * 5


def test_track_chain_runs_into_the_frame_border():
    frames, jobs, grid, radius = _cached("border", eu.border_case)
    got = _assert_same(frames, jobs, grid, radius)
    t, l = jobs[0][1], jobs[0][4]
    for oy, ox, _, _ in got[0].tolist():
        t, l = t + oy, l + ox
        assert 0 <= t and t + 36 <= 96 and 0 <= l and l + 34 <= 128


def test_track_chain_largest_configuration():
    """grid 64 with radius 32 on three-step chains: the largest LDS footprint and the most candidates"""
    frames, jobs, grid, radius = _cached("large", eu.large_case)
    assert (grid, radius) == (64, 32) and all(j[7] == 3 for j in jobs)
    _assert_same(frames, jobs, grid, radius)


def test_track_chain_split_in_two_launches_equals_one():
    for key, case in (("moving", eu.moving_case), ("border", eu.border_case)):
        frames, jobs, grid, radius = _cached(key, case)
        jobs = [j for j in jobs if j[7] >= 3]
        dev = torch.as_tensor(frames).cuda()
        whole = _lib.track_chain(dev, jobs, grid=grid, radius=radius).cpu()
        head, _ = eu.split(jobs, 2, [(0, 0)] * len(jobs))
        first = _lib.track_chain(dev, head, grid=grid, radius=radius).cpu()
        _, tail = eu.split(jobs, 2, first[:, :, :2].sum(1).tolist())
        assert any(t[8] or t[9] for t in tail)
        second = _lib.track_chain(dev, tail, grid=grid, radius=radius).cpu()
        for n, j in enumerate(jobs):
            assert torch.equal(torch.cat([first[n], second[n, :j[7] - 2]]), whole[n, :j[7]])


@pytest.mark.parametrize("grid", [16, 32])
def test_one_step_chains_equal_track_match(grid):
    frames, jobs = _cached(("random", grid), lambda: eu.random_case(grid))
    dev = _cached(("dev", id(frames)), lambda: torch.as_tensor(frames).cuda())
    ones = [(*j[:7], 1, j[8], j[9], eu.STOP_NEVER) for j in jobs]
    for radius in (0, 5, 8):
        chain = _lib.track_chain(dev, ones, grid=grid, radius=radius)
        match = _lib.track_match(dev, eu.match_rows(ones), grid=grid, radius=radius)
        assert tuple(chain.shape) == (len(jobs), 1, 4) and torch.equal(chain[:, 0], match)


def test_track_chain_refusals_bad_rows_and_no_jobs():
    frames, jobs, grid, radius = _cached("moving", eu.moving_case)
    dev = torch.as_tensor(frames).cuda()
    none = _lib.track_chain(dev, [], grid=16, radius=4)
    assert tuple(none.shape) == (0, 0, 4) and none.dtype == torch.int32 and none.is_cuda
    for kw in (dict(grid=8), dict(grid=48), dict(grid=128), dict(radius=-1), dict(radius=33)):
        with pytest.raises(_lib.GenConViTHipError):
            _lib.track_chain(dev, jobs, **{"grid": 16, "radius": 4, **kw})
    edit = lambda row, **kw: tuple(kw.get(f"c{i}", v) for i, v in enumerate(row))
    bad = [edit(jobs[0], c0=6), edit(jobs[0], c5=-1), edit(jobs[0], c7=6), edit(jobs[1], c7=6),     # frame indices
           edit(jobs[0], c3=97), edit(jobs[0], c4=-1), edit(jobs[0], c8=-21), edit(jobs[0], c9=89),  # outside the frame
           edit(jobs[0], c3=35), edit(jobs[0], c6=0), edit(jobs[0], c6=2), edit(jobs[0], c7=0),
           edit(jobs[0], c7=1025), edit(jobs[0], c10=-1)]
    for row in bad:
        with pytest.raises(_lib.GenConViTHipError):
            _lib.track_chain(dev, [row], grid=16, radius=4)
    with pytest.raises(_lib.GenConViTHipError):
        _lib.track_chain(dev, jobs, grid=64, radius=4)                        # a 48 x 40 template on a grid of 64
    with pytest.raises(_lib.GenConViTHipError):
        _lib.track_chain(dev.cpu(), jobs, grid=16, radius=4)                  # a host tensor never reaches a launch
    # the launcher's own checks, through the C ABI: bad scalars are refused with a reason and nothing is launched
    lib = _lib.load()
    rows = [jobs[0], bad[0], bad[7], jobs[1], bad[10], bad[12], bad[13], bad[3]]
    jd = torch.as_tensor(rows, dtype=torch.int32).cuda()
    out = torch.full((len(rows), 5, 4), -7, dtype=torch.int32, device="cuda")
    stream = _lib.current_stream_ptr(dev.device)
    call = lambda nf=6, h=96, w=128, n=len(rows), steps=5, grid=16, radius=5: lib.gcv_track_chain(
        dev.data_ptr(), nf, h, w, jd.data_ptr(), n, steps, grid, radius, out.data_ptr(), stream)
    for kw in (dict(grid=8), dict(grid=0), dict(grid=65), dict(radius=-1), dict(radius=33), dict(steps=0), dict(steps=1025),
               dict(nf=0), dict(h=0), dict(w=-1)):
        assert call(**kw) != 0 and _lib.last_error()
        with pytest.raises(_lib.GenConViTHipError):
            _lib.check(call(**kw), "gcv_track_chain")
    assert call(n=0) == 0
    torch.cuda.synchronize()
    assert bool((out == -7).all())                                            # nothing was launched so far
    # rows the binding would refuse write the refusal row throughout and read nothing; their neighbours are served
    assert call() == 0
    want = eu.track_chain_ref(frames, jobs, 16, 5)
    got = out.cpu()
    assert got[0].tolist() == want[0].tolist() and got[3].tolist() == want[1].tolist()
    for n in (1, 2, 4, 5, 6, 7):
        assert got[n].tolist() == [list(eu.NONE)] * 5
    # and a valid call after all that is correct
    _assert_same(frames, jobs, grid, radius)


# ----------------------------------------------------------------------------- scan_frames(extend=True) end to end
def _ensemble():
    """the fp16 ensemble of tests/test_scan_gpu.py: the same cached networks, built once per session"""
    from tests.test_scan_gpu import _ed, _vae
    return GenConViT.from_modules(_ed(torch.float16), _vae(torch.float16), net="genconvit")


def test_scan_frames_extend_on_the_device():
    """the moving pattern, seen by the detector in frame 2 only: the track is carried back to frame 0 and on to frame 5 by
    the restatement's steps, host frames (two groups of at most 4 frames) and device frames (one launch) agree, and the
    scores are those of a scan that is given the extended boxes as detections"""
    frames, _, grid, radius = _cached("moving", eu.moving_case)
    t, l = eu.MOVE_PATH[2]
    det = [(2, t, l + eu.MOVE_W, t + eu.MOVE_H, l)]
    model = _ensemble()
    eps = synth.make_eps(6, name="extend").cuda()
    args = dict(grid=grid, radius=radius, steps=8, cost_max=40.0)
    stop = int(40.0 * grid * grid)
    res = pred_func.scan_frames(frames, model, boxes=det, detect_every=4, window=4, stride=2, eps=eps, max_batch=4,
                                extend=True, extend_args=args)
    want = eu.track_chain_ref(frames, [(*det[0], 3, 1, 3, 0, 0, stop), (*det[0], 1, -1, 2, 0, 0, stop)], grid, radius)
    assert (want[0, :, 2] >= 0).all() and (want[1, :2, 2] >= 0).all()
    assert [b[0] for b in res["tracks"][0]] == list(range(6)) and res["tracks"][0][2] == det[0]
    assert res["extend"].dtype == np.int32 and res["extend"][:, :3].tolist() == [[0, 3, 1], [0, 4, 1], [0, 5, 1], [0, 1, -1],
                                                                               [0, 0, -1]]
    assert res["extend"][:3, 3:].tolist() == want[0].tolist() and res["extend"][3:, 3:].tolist() == want[1, :2].tolist()
    box = det[0]
    for f, (oy, ox) in zip((3, 4, 5), want[0, :, :2].tolist()):
        box = (f, box[1] + oy, box[2] + ox, box[3] + oy, box[4] + ox)
        assert res["tracks"][0][f] == box
    again = pred_func.scan_frames(frames, model, boxes=res["boxes"], detect_every=1, window=4, stride=2, eps=eps, max_batch=4)
    assert again["tracks"] == res["tracks"] and "extend" not in again
    assert torch.equal(again["frame_scores"], res["frame_scores"]) and again["windows"] == res["windows"]
    dev = pred_func.scan_frames(torch.as_tensor(frames).cuda(), model, boxes=det, detect_every=4, window=4, stride=2, eps=eps,
                                max_batch=4, extend=True, extend_args=args)
    assert dev["tracks"] == res["tracks"] and (dev["extend"] == res["extend"]).all()
    assert torch.equal(dev["frame_scores"], res["frame_scores"])
