"""``gcv_frame_cells``, ``gcv_blend_fit`` and ``gcv_hist_diff_lag`` on the MI355X, bit for bit against their CPU restatement
(tests/transutil.py: ``torch.equal``, no tolerance — the arithmetic is integer), their refusals, and
``pred_func.shot_transitions`` / ``scan_frames(transitions=True)`` end to end with synthetic weights."""
import pytest
import torch

from genconvit_amd import _lib, synth
from genconvit_amd.model import pred_func
from genconvit_amd.model.genconvit import GenConViT
from tests import cutsutil as cu
from tests import transutil as tu

pytestmark = pytest.mark.gpu
torch.set_grad_enabled(False)

_CACHE = {}
GRIDS = [8, 16, 32]


def _cached(key, make):
    if key not in _CACHE:
        _CACHE[key] = make()
    return _CACHE[key]


def _video(name, make=None):
    """(host frames, the same on the device), made once"""
    frames = _cached(name, make or getattr(tu, name, None) or getattr(cu, name))
    return frames, _cached((name, "dev"), lambda: torch.as_tensor(frames).cuda())


def _cells_ref(name, frames, grid):
    return _cached((name, "cells", grid), lambda: torch.as_tensor(tu.frame_cells_ref(frames, grid)))


def _assert_cells(frames, dev, grid, want=None):
    """the cells of ``dev`` (a device tensor that holds ``frames``) equal the restatement; returns them"""
    cells = _lib.frame_cells(dev, grid)
    assert cells.is_cuda and cells.dtype == torch.int32 and tuple(cells.shape) == (frames.shape[0], grid * grid)
    want = torch.as_tensor(tu.frame_cells_ref(frames, grid)) if want is None else want
    got = cells.cpu().long()
    if not torch.equal(got, want):
        bad = (got != want).nonzero()
        f, c = bad[0].tolist()
        raise AssertionError(f"grid {grid}: {len(bad)} cells differ; first: frame {f} cell ({c // grid}, {c % grid}) got "
                             f"{int(got[f, c])} want {int(want[f, c])}")
    return cells


# ----------------------------------------------------------------------------- frame_cells
@pytest.mark.parametrize("grid", GRIDS)
def test_cells_of_the_transition_video(grid):
    """15 x 90 x 130: 390 bytes a row, sides divisible by neither 4 nor 8; at G = 32 the cells are 2-3 x 4-5 pixels, so a
    lane's 4-pixel group crosses cell edges.  One workgroup per row of cells (plain stores)."""
    frames, dev = _video("transition_video")
    _assert_cells(frames[:15], dev[:15], grid, _cells_ref("transition_video", frames, grid)[:15])


@pytest.mark.parametrize("grid", GRIDS)
def test_noise_and_an_odd_base_pointer(grid):
    """4 x 37 x 53 uniform noise (at G = 32 a cell is 1-2 x 1-2 pixels: a group holds two whole cells), and the same video
    from its second frame on: that slice starts 5 883 bytes in, so the rows start at every byte offset of a dword"""
    frames, dev = _video("noise_video")
    _assert_cells(frames, dev, grid)
    tail = dev[1:]
    assert tail.data_ptr() % 2 == 1 and tail.is_contiguous()
    _assert_cells(frames[1:], tail, grid)
    _assert_cells(frames[3:], dev[3:], grid)                                    # the last frame: the buffer's last bytes


def test_one_pixel_per_cell():
    frames, dev = _video("tiny", tu.tiny_video)
    cells = _assert_cells(frames, dev, 32)
    assert torch.equal(cells.cpu().long(), torch.as_tensor(cu.luma(frames)).reshape(2, -1))


def test_many_frames_take_the_unsplit_path():
    """70 frames of 37 x 53 at G = 16 are 1 120 rows of cells: one workgroup each, plain stores, rows of 2-3 pixel rows"""
    frames, dev = _video("many", cu.many_video)
    assert tu.cells_slices(70, 37, 16) == 1
    _assert_cells(frames, dev, 16)


@pytest.mark.parametrize("grid", [8, 32])
def test_rows_wider_than_a_workgroup(grid):
    """1 x 37 x 1103: 276 groups a row, more than the 256 threads — a thread's next group is in the same pixel row"""
    frames, dev = _video("wide", tu.wide_video)
    _assert_cells(frames, dev, grid)


def test_tall_frames_take_the_split_path():
    """few frames of many rows: a row of cells is split over several workgroups, merged by atomic adds into a zeroed
    output.  1 x 512 x 512 flat 255 at G = 8 (8 slices of 8 pixel rows): every cell is exactly 255 * 4096; 2 x 161 x 53
    noise at G = 8 (2 slices of the 20-21 rows, 10 and 10-11)."""
    flat = _cached("flat", tu.flat_video)
    assert tu.cells_slices(1, 512, 8) == 8 and tu.cells_slices(2, 161, 8) == tu.cells_slices(1, 161, 8) == 2
    cells = _assert_cells(flat, torch.as_tensor(flat).cuda(), 8)
    assert bool((cells == 255 * 4096).all())
    frames, dev = _video("tall", tu.tall_video)
    _assert_cells(frames, dev, 8)
    _assert_cells(frames[1:], dev[1:], 8)


# ----------------------------------------------------------------------------- blend_fit
def _assert_fit(cells_host, lag):
    got = _lib.blend_fit(torch.as_tensor(cells_host, dtype=torch.int32).cuda(), lag)
    want = torch.as_tensor(tu.blend_fit_ref(cells_host, lag))
    assert got.is_cuda and got.dtype == torch.int64 and tuple(got.shape) == tuple(want.shape)
    if not torch.equal(got.cpu(), want):
        bad = (got.cpu() != want).nonzero()
        p, c = bad[0].tolist()
        raise AssertionError(f"lag {lag}: {len(bad)} sums differ; first: span {p} column {c} got {int(got[p, c])} want "
                             f"{int(want[p, c])}")
    return got


@pytest.mark.parametrize("grid", GRIDS)
def test_fits_of_the_transition_video(grid):
    """G = 8: one wave a span; G = 16: four waves, a cell a thread; G = 32: four cells a thread"""
    frames, _ = _video("transition_video")
    cells = _cells_ref("transition_video", frames, grid).numpy()
    for lag in (2, 4, 8, 32):
        _assert_fit(cells, lag)


@pytest.mark.parametrize("grid", [16, 32])
def test_fits_beyond_float64_across_waves_and_cells_of_a_thread(grid):
    """the sums near 2^63 at G = 16 (four waves, summed in 64 bits through LDS) and G = 32 (four cells a thread as well)"""
    cells = tu.extreme_cells(grid)
    for lag in (2, 3, 5):
        fit = _assert_fit(cells, lag)
        assert int(fit.max()) > 2 ** 62 and tuple(fit.shape) == (6 - lag, 2 * lag - 1)


def test_fits_beyond_float64_and_the_shortest_inputs():
    cells = tu.extreme_cells()
    for lag in (2, 3, 5):
        fit = _assert_fit(cells, lag)
        assert int(fit.max()) > 2 ** 62 and tuple(fit.shape) == (6 - lag, 2 * lag - 1)      # lag = 5 = F - 1: one span
    d = torch.as_tensor(cells).cuda()
    assert tuple(_lib.blend_fit(d[:5], 5).shape) == (0, 9) and tuple(_lib.blend_fit(d[:2], 6).shape) == (0, 11)
    lib, stream = _lib.load(), _lib.current_stream_ptr(d.device)
    out = torch.full((64,), -7, dtype=torch.int64, device="cuda")
    assert lib.gcv_blend_fit(d.data_ptr(), 5, 8, 5, out.data_ptr(), stream) == 0              # lag = F: nothing is written
    assert lib.gcv_blend_fit(None, 3, 8, 5, None, stream) == 0
    torch.cuda.synchronize()
    assert bool((out == -7).all())


# ----------------------------------------------------------------------------- hist_diff_lag
@pytest.mark.parametrize("regions", [1, 4])
def test_lagged_histogram_distances(regions):
    frames, dev = _video("three_shot_video")
    hist = _lib.frame_hist(dev, regions)
    ref = cu.frame_hist_ref(frames, regions)
    for lag in (1, 4, 8, 14):
        dist = _lib.hist_diff_lag(hist, lag)
        assert dist.is_cuda and dist.dtype == torch.int32 and tuple(dist.shape) == (15 - lag, regions * regions)
        assert torch.equal(dist.cpu().long(), torch.as_tensor(tu.hist_diff_lag_ref(ref, lag)))
    assert torch.equal(_lib.hist_diff_lag(hist, 1), _lib.hist_diff(hist))
    assert tuple(_lib.hist_diff_lag(hist, 15).shape) == (0, regions * regions)
    assert tuple(_lib.hist_diff_lag(hist, 40).shape) == (0, regions * regions)


# ----------------------------------------------------------------------------- refusals
def test_refusals_and_a_valid_call_after_them():
    frames, dev = _video("noise_video")
    err = _lib.GenConViTHipError
    for bad in (0, 4, 12, 64, 16.0, True, None):
        with pytest.raises(err):
            _lib.frame_cells(dev, bad)
    for bad in (dev.cpu(), dev.float(), dev[..., :2], dev[:0], dev[0]):
        with pytest.raises(err):
            _lib.frame_cells(bad, 8)
    with pytest.raises(err):
        _lib.frame_cells(dev[:, :31], 32)                                       # H = 31 < grid
    with pytest.raises(err):
        _lib.frame_cells(dev[:, :, :15].contiguous(), 16)                       # W = 15 < grid
    for bad in (torch.empty((4, 64), dtype=torch.int32), torch.empty((3, 64), dtype=torch.int32).cuda(),
                torch.empty((4, 64), dtype=torch.int64).cuda(), torch.empty((64, 4), dtype=torch.int32).cuda().t()):
        with pytest.raises(err):
            _lib.frame_cells(dev, 8, out=bad)
    good = _lib.frame_cells(dev, 8)
    for bad in (good.cpu(), good.long(), good[:, :60], good[0], good.reshape(4, 8, 8)):
        with pytest.raises(err):
            _lib.blend_fit(bad, 2)
    for bad in (1, 0, -2, 33, 2.0, True, None):
        with pytest.raises(err):
            _lib.blend_fit(good, bad)
    hist = _lib.frame_hist(dev, 4)
    for bad in (hist.cpu(), hist.float(), hist[:, :3], hist[0]):
        with pytest.raises(err):
            _lib.hist_diff_lag(bad, 2)
    for bad in (0, -1, 2.0, True, None):
        with pytest.raises(err):
            _lib.hist_diff_lag(hist, bad)
    # the launchers' own checks, through the C ABI: bad scalars are refused with a reason and nothing is written
    lib, stream = _lib.load(), _lib.current_stream_ptr(dev.device)
    out = torch.full((4, 1200), -7, dtype=torch.int32, device="cuda")
    call = lambda nf=4, h=37, w=53, g=8: lib.gcv_frame_cells(dev.data_ptr(), nf, h, w, g, out.data_ptr(), stream)
    for kw in (dict(g=0), dict(g=4), dict(g=12), dict(g=64), dict(g=-8), dict(nf=0), dict(nf=-1), dict(h=0), dict(w=-1),
               dict(h=31, g=32), dict(w=15, g=16), dict(h=1 << 13, w=(1 << 12) + 1)):          # the last: 2^25 + 2^13 pixels
        assert call(**kw) != 0 and _lib.last_error()
        with pytest.raises(err):
            _lib.check(call(**kw), "gcv_frame_cells")
    assert lib.gcv_frame_cells(None, 4, 37, 53, 8, out.data_ptr(), stream) != 0
    assert lib.gcv_frame_cells(dev.data_ptr(), 4, 37, 53, 8, None, stream) != 0
    fout = torch.full((64,), -7, dtype=torch.int64, device="cuda")
    fit = lambda nf=4, g=8, lag=2: lib.gcv_blend_fit(good.data_ptr(), nf, g, lag, fout.data_ptr(), stream)
    for kw in (dict(lag=1), dict(lag=0), dict(lag=-3), dict(lag=33), dict(g=4), dict(g=0), dict(g=64), dict(nf=0), dict(nf=-2)):
        assert fit(**kw) != 0 and _lib.last_error()
    assert lib.gcv_blend_fit(None, 4, 8, 2, fout.data_ptr(), stream) != 0
    assert lib.gcv_blend_fit(good.data_ptr(), 4, 8, 2, None, stream) != 0
    dout = torch.full((4, 64), -7, dtype=torch.int32, device="cuda")
    diff = lambda nf=4, r=4, lag=2: lib.gcv_hist_diff_lag(hist.data_ptr(), nf, r, lag, dout.data_ptr(), stream)
    for kw in (dict(r=0), dict(r=3), dict(r=16), dict(nf=0), dict(nf=-2), dict(lag=0), dict(lag=-1)):
        assert diff(**kw) != 0 and _lib.last_error()
    assert lib.gcv_hist_diff_lag(None, 4, 4, 2, dout.data_ptr(), stream) != 0
    assert lib.gcv_hist_diff_lag(hist.data_ptr(), 4, 4, 2, None, stream) != 0
    assert diff(lag=4) == 0 and fit(lag=4) == 0                                 # no span: no launch
    torch.cuda.synchronize()
    assert bool((out == -7).all()) and bool((fout == -7).all()) and bool((dout == -7).all())      # nothing was written so far
    # the same entries with good scalars write exactly their elements
    assert call() == 0 and fit() == 0 and diff() == 0
    want = torch.as_tensor(tu.frame_cells_ref(frames, 8))
    assert torch.equal(out.cpu().flatten()[:256].long(), want.flatten()) and bool((out.flatten()[256:] == -7).all())
    assert torch.equal(fout.cpu()[:6], torch.as_tensor(tu.blend_fit_ref(want, 2)).flatten()) and bool((fout[6:] == -7).all())
    assert torch.equal(dout.cpu().flatten()[:32].long(), torch.as_tensor(tu.hist_diff_lag_ref(hist.cpu(), 2)).flatten())
    assert bool((dout.flatten()[32:] == -7).all())
    # out= writes a group's rows of a larger buffer and nothing else, on the plain and on the split path
    buf = torch.full((6, 64), -7, dtype=torch.int32, device="cuda")
    assert _lib.frame_cells(dev, 8, out=buf[1:5]).data_ptr() == buf[1:5].data_ptr()
    assert torch.equal(buf[1:5].cpu().long(), want) and bool((buf[0] == -7).all()) and bool((buf[5] == -7).all())
    tall, tall_dev = _video("tall", tu.tall_video)
    buf.fill_(-7)
    _lib.frame_cells(tall_dev, 8, out=buf[2:4])
    assert torch.equal(buf[2:4].cpu().long(), torch.as_tensor(tu.frame_cells_ref(tall, 8)))
    assert bool((buf[:2] == -7).all()) and bool((buf[4:] == -7).all())
    # and valid calls after all that are correct
    for grid in GRIDS:
        _assert_cells(frames, dev, grid)


# ----------------------------------------------------------------------------- shot_transitions
def test_shot_transitions_on_device_and_host_frames():
    frames, dev = _video("transition_video")
    want, want_info = _cached("transitions", lambda: tu.transitions_ref(frames))
    assert want == [(8, 13), (30, 34)]
    for given, kw in ((dev, {}), (frames, dict(max_frames=4, dev="cuda")), (torch.as_tensor(frames), dict(max_frames=37, dev="cuda"))):
        got, info = pred_func.shot_transitions(given, **kw)
        assert got == want and tu.same_info(info, want_info)
    ref = tu.transitions_ref(frames, grid=32, lags=(3, 6), regions=2)
    got, info = pred_func.shot_transitions(dev, grid=32, lags=(3, 6), regions=2)
    assert got == ref[0] and tu.same_info(info, ref[1])
    for name in ("three_shot_video",):
        assert pred_func.shot_transitions(_video(name)[1])[0] == []
    pan, pan_dev = _video("pan", lambda: tu.pan_video(2))
    got, info = pred_func.shot_transitions(pan_dev)
    assert got == [] and tu.same_info(info, tu.transitions_ref(pan)[1])


# ----------------------------------------------------------------------------- scan_frames(transitions=True) end to end
def _ensemble():
    """the fp16 ensemble of tests/test_scan_gpu.py: the same cached networks, built once per session"""
    from tests.test_scan_gpu import _ed, _vae
    return GenConViT.from_modules(_ed(torch.float16), _vae(torch.float16), net="genconvit")


def _touches(first, last, transitions):
    return any(first <= b and a <= last for a, b in transitions)


def test_scan_frames_transitions_on_the_device():
    """one box on all 38 frames of the transition video: IoU alone makes it one track; the transitions and the cut make it
    four, and the 11 frames inside the dissolve and the fade are not scored.  The crops that remain run as they would in a
    plain scan of those boxes, so their scores are bit-equal to it."""
    frames, dev = _video("transition_video")
    want, want_info = _cached("transitions", lambda: tu.transitions_ref(frames))
    boxes = [(f, *cu.FACE_BOX) for f in range(38)]
    keep = [f for f in range(38) if not _touches(f, f, want)]
    model = _ensemble()
    eps = synth.make_eps(38, name="transitions").cuda()
    kw = dict(window=3, stride=1, max_batch=6)
    res = pred_func.scan_frames(frames, model, boxes=boxes, eps=eps[keep], transitions=True, cuts=True, **kw)
    assert res["transitions"] == want == [(8, 13), (30, 34)] and tu.same_info(res["transition_info"], want_info)
    assert tu.HARD_CUT in res["cuts"]
    spans = [(t[0][0], t[-1][0]) for t in res["tracks"]]
    assert {7, 21, 29} <= {b for _, b in spans} and {14, 22} <= {a for a, _ in spans}
    assert [b[0] for b in res["boxes"]] == keep and len(keep) == 27
    assert not any(_touches(a, b, want) for a, b in spans)
    assert not any(_touches(w[1], w[2], want) for w in res["windows"]) and res["windows"]
    assert not any(_touches(s[1], s[2], want) for s in res["segments"])
    plain = pred_func.scan_frames(frames, model, boxes=[boxes[f] for f in keep], eps=eps[keep], **kw)
    assert "transitions" not in plain and [b[0] for b in plain["boxes"]] == keep
    assert torch.equal(res["frame_scores"], plain["frame_scores"])
    whole = pred_func.scan_frames(frames, model, boxes=boxes, eps=eps, **kw)
    assert whole["tracks"] == [boxes] and any(_touches(w[1], w[2], want) for w in whole["windows"])
    # device frames: the cells and histograms in place, the same answer
    on_dev = pred_func.scan_frames(dev, model, boxes=boxes, eps=eps[keep], transitions=True, cuts=True, **kw)
    for key in ("transitions", "cuts", "tracks", "boxes", "windows", "segments", "track_verdicts", "verdict"):
        assert on_dev[key] == res[key]
    assert tu.same_info(on_dev["transition_info"], res["transition_info"])
    assert (on_dev["cut_scores"] == res["cut_scores"]).all()
    assert torch.equal(on_dev["frame_scores"], res["frame_scores"])
    assert torch.equal(on_dev["window_means"], res["window_means"])
