"""``gcv_frame_hist`` and ``gcv_hist_diff`` on the MI355X, bit for bit against their CPU restatement (tests/cutsutil.py:
``torch.equal``, no tolerance — the arithmetic is integer), their refusals, and ``pred_func.shot_cuts`` /
``scan_frames(cuts=True)`` end to end with synthetic weights."""
import numpy as np
import pytest
import torch

from genconvit_amd import _lib, synth
from genconvit_amd.model import pred_func
from genconvit_amd.model.genconvit import GenConViT
from tests import cutsutil as cu

pytestmark = pytest.mark.gpu
torch.set_grad_enabled(False)

_CACHE = {}
REGIONS = [1, 2, 4, 8]


def _cached(key, make):
    if key not in _CACHE:
        _CACHE[key] = make()
    return _CACHE[key]


def _video(name):
    """(host frames, the same on the device), made once"""
    frames = _cached(name, getattr(cu, name))
    return frames, _cached((name, "dev"), lambda: torch.as_tensor(frames).cuda())


def _assert_same(frames, dev, regions):
    """hist and dist of ``dev`` (a device tensor that holds ``frames``) equal the restatement; returns both"""
    hist = _lib.frame_hist(dev, regions)
    nf, h, w = frames.shape[:3]
    assert hist.is_cuda and hist.dtype == torch.int32 and tuple(hist.shape) == (nf, regions * regions, 64)
    want = torch.as_tensor(cu.frame_hist_ref(frames, regions))
    if not torch.equal(hist.cpu(), want):
        bad = (hist.cpu() != want).nonzero()
        f, r, b = bad[0].tolist()
        raise AssertionError(f"regions {regions}: {len(bad)} counts differ; first: frame {f} region {r} bin {b} got "
                             f"{int(hist[f, r, b])} want {int(want[f, r, b])}")
    assert torch.equal(hist.sum(-1).cpu(), torch.as_tensor(cu.region_pixels(h, w, regions)).expand(nf, -1))
    dist = _lib.hist_diff(hist)
    assert dist.is_cuda and dist.dtype == torch.int32 and tuple(dist.shape) == (nf - 1, regions * regions)
    assert torch.equal(dist.cpu().long(), torch.as_tensor(cu.hist_diff_ref(want)))
    return hist, dist


@pytest.mark.parametrize("regions", REGIONS)
def test_three_shot_video(regions):
    """15 x 90 x 130: 390 bytes a row, sides divisible by neither 4 nor 8; at R = 1, 2, 4 the regions are split over
    several workgroups and merged by atomic adds, at R = 8 each has its own"""
    frames, dev = _video("three_shot_video")
    _assert_same(frames, dev, regions)
    want = cu.scores_ref(cu.hist_diff_ref(cu.frame_hist_ref(frames, regions)), 90, 130, regions)
    for given in (dev, frames):                             # in place on the device; host frames in groups of 4
        cuts, scores = pred_func.shot_cuts(given, regions=regions, max_frames=4, dev="cuda")
        assert cuts == [5, 9] and scores.dtype == np.float64 and (scores == want).all()
    inside = [s for p, s in enumerate(want) if p + 1 not in (5, 9)]
    assert max(inside) < 0.1 and want[4] > 0.5 and want[8] > 0.5


@pytest.mark.parametrize("regions", REGIONS)
def test_noise_and_an_odd_base_pointer(regions):
    """4 x 37 x 53 uniform noise (at R = 8 a region is 4-5 x 6-7 pixels, less than a wave), and the same video from its
    second frame on: that slice starts 5 883 bytes in, so the rows start at every byte offset of a dword"""
    frames, dev = _video("noise_video")
    _assert_same(frames, dev, regions)
    tail = dev[1:]
    assert tail.data_ptr() % 2 == 1 and tail.is_contiguous()
    _assert_same(frames[1:], tail, regions)
    last = dev[3:]                                          # one frame: the slices of one region, and no pair
    hist = _assert_same(frames[3:], last, regions)[0]
    assert tuple(_lib.hist_diff(hist).shape) == (0, regions * regions)


def test_many_frames_take_the_unsplit_path_at_every_size():
    """70 frames of 37 x 53 at R = 4 are 1 120 regions: one workgroup each, plain stores, regions of 9-10 rows"""
    frames = _cached("many", cu.many_video)
    assert cu.hist_slices(70, 37, 4) == 1
    _assert_same(frames, torch.as_tensor(frames).cuda(), 4)


def test_one_pixel_per_region():
    frames = _cached("tiny", cu.tiny_video)
    hist, dist = _assert_same(frames, torch.as_tensor(frames).cuda(), 8)
    assert int(hist.max()) == 1 and set(dist.flatten().tolist()) <= {0, 2}


@pytest.mark.parametrize("regions", [1, 4])
def test_flat_frames_fill_one_bin(regions):
    """2 x 260 x 260, flat 200 and flat 17: at R = 1 one bin holds 67 600 (more than 16 bits) and every lane of every wave
    adds to it; the histograms are disjoint, so dist is twice the pixel count"""
    frames, dev = _video("flat_pair")
    hist, dist = _assert_same(frames, dev, regions)
    n = cu.region_pixels(260, 260, regions)
    assert hist[0, :, 200 >> 2].tolist() == n.tolist() and hist[1, :, 17 >> 2].tolist() == n.tolist()
    assert dist.tolist() == [(2 * n).tolist()]
    if regions == 1:
        assert int(hist.max()) == 67600 and dist.tolist() == [[135200]]


@pytest.mark.parametrize("regions", [1, 2])
def test_the_first_and_the_last_bin(regions):
    """2 x 16 x 24, white, then black with every third column white: bins 0 and 63 hold everything (noise almost never
    reaches Y >= 252), and bin 63 is the last lane of hist_diff's wave"""
    frames, dev = _video("ends_pair")
    hist, dist = _assert_same(frames, dev, regions)
    n = cu.region_pixels(16, 24, regions)
    assert hist[0, :, 63].tolist() == n.tolist() and hist[1, :, 63].tolist() == (n // 3).tolist()
    assert hist[1, :, 0].tolist() == (n - n // 3).tolist() and dist.tolist() == [(2 * (n - n // 3)).tolist()]


@pytest.mark.parametrize("regions", [1, 2])
def test_columns_that_alternate_between_two_bins(regions):
    frames, dev = _video("striped_pair")
    hist, dist = _assert_same(frames, dev, regions)
    n = cu.region_pixels(64, 96, regions)
    assert hist[0, :, 10].tolist() == n.tolist()                           # 40 and 41 share bin 10
    assert hist[1, :, 10].tolist() == (n // 2).tolist() and hist[1, :, 62].tolist() == (n // 2).tolist()
    assert dist.tolist() == [n.tolist()]


def test_refusals_and_a_valid_call_after_them():
    frames, dev = _video("noise_video")
    for bad in (0, 3, 16, 4.0, True, None):
        with pytest.raises(_lib.GenConViTHipError):
            _lib.frame_hist(dev, bad)
    with pytest.raises(_lib.GenConViTHipError):
        _lib.frame_hist(dev.cpu(), 4)                                           # a host tensor never reaches a launch
    with pytest.raises(_lib.GenConViTHipError):
        _lib.frame_hist(dev.float(), 4)
    with pytest.raises(_lib.GenConViTHipError):
        _lib.frame_hist(dev[..., :2], 4)
    with pytest.raises(_lib.GenConViTHipError):
        _lib.frame_hist(dev[:0], 4)
    with pytest.raises(_lib.GenConViTHipError):
        _lib.frame_hist(dev[:, :7], 8)                                          # H = 7 < regions
    with pytest.raises(_lib.GenConViTHipError):
        _lib.frame_hist(dev[:, :, :3].contiguous(), 4)                          # W = 3 < regions
    good = _lib.frame_hist(dev, 4)
    for bad in (good.cpu(), good.float(), good[:, :3], good[:, :, :32], good[0], torch.zeros((4, 9, 64), dtype=torch.int32).cuda()):
        with pytest.raises(_lib.GenConViTHipError):
            _lib.hist_diff(bad)
    for bad in (torch.empty((4, 16, 64), dtype=torch.int32), torch.empty((3, 16, 64), dtype=torch.int32).cuda(),
                torch.empty((4, 16, 64), dtype=torch.int64).cuda(), torch.empty((4, 64, 16), dtype=torch.int32).cuda().transpose(1, 2)):
        with pytest.raises(_lib.GenConViTHipError):
            _lib.frame_hist(dev, 4, out=bad)
    # the launchers' own checks, through the C ABI: bad scalars are refused with a reason and nothing is written
    lib = _lib.load()
    stream = _lib.current_stream_ptr(dev.device)
    out = torch.full((4, 64, 64), -7, dtype=torch.int32, device="cuda")
    call = lambda nf=4, h=37, w=53, r=4: lib.gcv_frame_hist(dev.data_ptr(), nf, h, w, r, out.data_ptr(), stream)
    for kw in (dict(r=0), dict(r=3), dict(r=16), dict(r=-4), dict(nf=0), dict(nf=-1), dict(h=0), dict(w=-1), dict(h=7, r=8),
               dict(w=3), dict(h=1 << 16, w=(1 << 14) + 1)):
        assert call(**kw) != 0 and _lib.last_error()
        with pytest.raises(_lib.GenConViTHipError):
            _lib.check(call(**kw), "gcv_frame_hist")
    assert lib.gcv_frame_hist(None, 4, 37, 53, 4, out.data_ptr(), stream) != 0
    assert lib.gcv_frame_hist(dev.data_ptr(), 4, 37, 53, 4, None, stream) != 0
    dout = torch.full((3, 64), -7, dtype=torch.int32, device="cuda")
    diff = lambda nf=4, r=4: lib.gcv_hist_diff(good.data_ptr(), nf, r, dout.data_ptr(), stream)
    for kw in (dict(r=0), dict(r=3), dict(r=16), dict(nf=0), dict(nf=-2)):
        assert diff(**kw) != 0 and _lib.last_error()
    assert lib.gcv_hist_diff(None, 4, 4, dout.data_ptr(), stream) != 0
    assert diff(nf=1) == 0                                                      # one frame: no pair, no launch
    torch.cuda.synchronize()
    assert bool((out == -7).all()) and bool((dout == -7).all())                 # nothing was written so far
    # the same entries with good scalars write exactly their elements
    assert call() == 0 and diff() == 0
    want = torch.as_tensor(cu.frame_hist_ref(frames, 4))
    assert torch.equal(out.cpu().flatten()[:want.numel()], want.flatten())
    assert bool((out.flatten()[want.numel():] == -7).all())
    assert torch.equal(dout.cpu().flatten()[:48].long(), torch.as_tensor(cu.hist_diff_ref(want)).flatten())
    assert bool((dout.flatten()[48:] == -7).all())
    # out= writes a group's rows of a larger buffer and nothing else
    buf = torch.full((6, 16, 64), -7, dtype=torch.int32, device="cuda")
    assert _lib.frame_hist(dev, 4, out=buf[1:5]).data_ptr() == buf[1:5].data_ptr()
    assert torch.equal(buf[1:5].cpu(), want) and bool((buf[0] == -7).all()) and bool((buf[5] == -7).all())
    # and valid calls after all that are correct
    for regions in REGIONS:
        _assert_same(frames, dev, regions)


# ----------------------------------------------------------------------------- scan_frames(cuts=True) end to end
def _ensemble():
    """the fp16 ensemble of tests/test_scan_gpu.py: the same cached networks, built once per session"""
    from tests.test_scan_gpu import _ed, _vae
    return GenConViT.from_modules(_ed(torch.float16), _vae(torch.float16), net="genconvit")


def _straddles(first, last, cuts):
    return any(first < c <= last for c in cuts)


def test_scan_frames_cuts_on_the_device():
    """one box on all 15 frames of the three-shot video: IoU alone makes it one track, the cuts make it three.  The crops
    are the same in the same order, so the scores of the frames are bit-equal to the scan without cuts; only the votes
    change."""
    frames, dev = _video("three_shot_video")
    boxes = [(f, *cu.FACE_BOX) for f in range(15)]
    model = _ensemble()
    kw = dict(boxes=boxes, window=3, stride=1, max_batch=6, eps=synth.make_eps(15, name="cuts").cuda())
    plain = pred_func.scan_frames(frames, model, **kw)
    assert plain["tracks"] == [boxes] and "cuts" not in plain
    res = pred_func.scan_frames(frames, model, cuts=True, **kw)
    assert res["cuts"] == [5, 9] and res["tracks"] == [boxes[:5], boxes[5:9], boxes[9:]]
    want = cu.scores_ref(cu.hist_diff_ref(cu.frame_hist_ref(frames, 4)), 90, 130, 4)
    assert (res["cut_scores"] == want).all()
    assert torch.equal(res["frame_scores"], plain["frame_scores"])
    assert [w[:3] for w in res["windows"]] == [(0, 0, 2), (0, 1, 3), (0, 2, 4), (1, 5, 7), (1, 6, 8),
                                               (2, 9, 11), (2, 10, 12), (2, 11, 13), (2, 12, 14)]
    assert not any(_straddles(w[1], w[2], res["cuts"]) for w in res["windows"])
    assert not any(_straddles(s[1], s[2], res["cuts"]) for s in res["segments"])
    assert any(_straddles(w[1], w[2], res["cuts"]) for w in plain["windows"])
    fp = res["frame_scores"].cpu().double()
    for k, (t, first, last, _, _) in enumerate(res["windows"]):            # a window's mean is over its own shot's frames
        assert (res["window_means"][k].cpu().double() - fp[first:last + 1].mean(0)).abs().max().item() <= 2e-6
    # device frames: the histograms in place, the same answer
    on_dev = pred_func.scan_frames(dev, model, cuts=True, **kw)
    assert on_dev["cuts"] == res["cuts"] and on_dev["tracks"] == res["tracks"] and on_dev["windows"] == res["windows"]
    assert (on_dev["cut_scores"] == res["cut_scores"]).all() and on_dev["segments"] == res["segments"]
    assert torch.equal(on_dev["frame_scores"], res["frame_scores"])
    assert torch.equal(on_dev["window_means"], res["window_means"])
