"""The device side of the whole-video scan on the MI355X: ``gcv_face_crop_preprocess`` bit for bit against the two launches
it replaces and against the CPU restatement, ``gcv_vote_windows`` against float64, and ``pred_func.scan_frames`` end to
end with synthetic weights against the per-crop path (``crop_faces`` -> ``preprocess_frame`` -> model -> sigmoid)."""
import numpy as np
import pytest
import torch

from genconvit_amd import _lib, synth
from genconvit_amd.model import pred_func
from genconvit_amd.model.config import load_config
from genconvit_amd.model.genconvit import GenConViT
from genconvit_amd.model.genconvit_ed import GenConViTED
from genconvit_amd.model.genconvit_vae import GenConViTVAE
from tests import scanutil as su
from tests.conftest import synthetic_sd

pytestmark = pytest.mark.gpu
torch.set_grad_enabled(False)

DTYPES = [torch.float32, torch.bfloat16, torch.float16]
_CACHE = {}


def _cached(key, make):
    if key not in _CACHE:
        _CACHE[key] = make()
    return _CACHE[key]


def _regime_case():
    """(frames on the device, boxes): the thirteen all-regime boxes over 4 x 720 x 1280 frames"""
    frames = _cached("regime frames", su.frames_all_regimes)
    return _cached("regime frames dev", lambda: torch.as_tensor(frames).cuda()), su.boxes_all_regimes(4, 720, 1280)


def _fuzz_case():
    frames, boxes = _cached("fuzz", su.fuzz_boxes)
    return _cached("fuzz dev", lambda: torch.as_tensor(frames).cuda()), boxes


# ----------------------------------------------------------------------------- gcv_face_crop_preprocess
def _assert_same_bits(frames, boxes, size, dtype):
    got = _lib.face_crop_preprocess(frames, boxes, size=size, dtype=dtype)
    want = _lib.preprocess(_lib.face_crop_resize(frames, boxes, size), dtype)
    assert got.dtype == dtype and tuple(got.shape) == (len(boxes), 3, size, size)
    if not torch.equal(got, want):
        bad = (got != want).flatten(1).any(1).nonzero().flatten().tolist()
        raise AssertionError(f"{dtype} size {size}: boxes {bad} differ, first {boxes[bad[0]]}")


@pytest.mark.parametrize("dtype", DTYPES)
def test_face_crop_preprocess_is_bit_equal_to_the_two_launches_in_every_regime(dtype):
    _assert_same_bits(*_regime_case(), 224, dtype)


@pytest.mark.parametrize("size", [224, 32])
@pytest.mark.parametrize("dtype", DTYPES)
def test_face_crop_preprocess_random_boxes_are_bit_equal_to_the_two_launches(dtype, size):
    _assert_same_bits(*_fuzz_case(), size, dtype)


def test_face_crop_preprocess_matches_the_cpu_restatement():
    """fp32 within 1e-6 and fp16 within 2e-3 of INTER_AREA restatement -> reference normalisation: the bounds of
    test_preprocess_frame_on_device_matches_reference_semantics (the crop itself is bit-equal, so nothing is added)."""
    frames, boxes = _regime_case()
    want = su.face_crop_preprocess_ref(frames, boxes)
    for dtype, tol in ((torch.float32, 1e-6), (torch.float16, 2e-3)):
        err = (_lib.face_crop_preprocess(frames, boxes, dtype=dtype).float().cpu() - want).abs().max().item()
        print(f"\nface_crop_preprocess {dtype}: max |diff vs CPU restatement| = {err:.3e} (bound {tol:g})")
        assert err <= tol


def test_face_crop_preprocess_boundary_cases():
    frames, _ = _fuzz_case()                                                  # 3 x 480 x 640
    for box in ((0, 10, 700, 100, 10), (3, 0, 10, 10, 0), (0, -1, 10, 10, 0), (0, 20, 10, 20, 0)):
        with pytest.raises(_lib.GenConViTHipError):
            _lib.face_crop_preprocess(frames, [box])
    for dtype in DTYPES:
        out = _lib.face_crop_preprocess(frames, [], size=32, dtype=dtype)
        assert tuple(out.shape) == (0, 3, 32, 32) and out.dtype == dtype and out.is_cuda
    with pytest.raises(_lib.GenConViTHipError):
        _lib.face_crop_preprocess(frames.cpu(), [(0, 0, 10, 10, 0)])


# ----------------------------------------------------------------------------- gcv_vote_windows
VOTE_TOL = 2e-6      # a CPU emulation of the two passes in fp32 (sigmoid, mean over nets, then a 64-lane strided sum with a
#                      tree or a sequential sum) stays within 1.9e-7 ~ 3 * 2^-24 of float64 on exactly these inputs; ten times
#                      that is left for the device's expf.  A wrong row or an off-by-one window moves a mean by ~1e-3.


def _logits(batch, nets, seed):
    x = 4.0 * torch.randn((nets * batch, 2), generator=torch.Generator().manual_seed(seed))
    x[3], x[7], x[batch - 1], x[nets * batch - 2] = 30.0, -30.0, 100.0, -100.0            # saturated: expf overflows to inf
    return x


def _extras(batch):
    """an empty range, a repeated one, a nested one, and ranges in reverse order"""
    return [(5, 5), (batch, batch), (0, 15), (0, 15), (3, 9), (20, batch), (10, 30), (0, 4)]


@pytest.mark.parametrize("nets", [1, 2])
@pytest.mark.parametrize("batch,windows", [(37, [(15, 1)]), (200, [(130, 7), (200, 1)])])
def test_vote_windows_matches_float64(batch, windows, nets):
    logits = _logits(batch, nets, 100 * batch + nets)
    ranges = [r for w, s in windows for r in pred_func.window_ranges(batch, w, s)]
    ranges = ranges + _extras(batch) + ranges[::-1]
    frame_p, mean2 = _lib.vote_windows(logits.cuda(), batch, nets, ranges)
    assert tuple(frame_p.shape) == (batch, 2) and tuple(mean2.shape) == (len(ranges), 2)
    assert frame_p.dtype == mean2.dtype == torch.float32
    want_p, want_m = su.vote_windows_ref(logits, batch, nets, ranges)
    ep = (frame_p.cpu().double() - want_p).abs().max().item()
    em = (mean2.cpu().double() - want_m).abs().max().item()
    print(f"\nvote_windows batch {batch} nets {nets}: {len(ranges)} ranges, max |diff vs float64| frame_p {ep:.3e} mean2 {em:.3e}")
    assert ep <= VOTE_TOL and em <= VOTE_TOL
    assert mean2[ranges.index((5, 5))].tolist() == [0.5, 0.5]


@pytest.mark.parametrize("nets", [1, 2])
def test_vote_windows_agrees_with_vote_segments_on_a_partition(nets):
    batch = 200
    logits = _logits(batch, nets, 7 + nets).cuda()
    offs = [0, 10, 10, 25, 160, batch]                                         # one empty segment, one longer than a wave
    seg = _lib.vote_segments(logits, batch, nets, torch.tensor(offs, dtype=torch.int32))
    _, mean2 = _lib.vote_windows(logits, batch, nets, list(zip(offs, offs[1:])))
    assert (seg - mean2).abs().max().item() <= VOTE_TOL
    frame_p, none = _lib.vote_windows(logits, batch, nets, [])               # the timeline alone
    assert tuple(none.shape) == (0, 2) and tuple(frame_p.shape) == (batch, 2)


def test_vote_windows_rejects_bad_ranges():
    logits = _logits(37, 2, 1).cuda()
    for bad in ((-1, 3), (0, 38), (5, 4)):
        with pytest.raises(_lib.GenConViTHipError):
            _lib.vote_windows(logits, 37, 2, [(0, 15), bad])
    with pytest.raises(_lib.GenConViTHipError):
        _lib.vote_windows(logits, 36, 2, [(0, 15)])                           # 74 rows are not 2 x 36
    with pytest.raises(_lib.GenConViTHipError):
        _lib.vote_windows(logits.cpu(), 37, 2, [(0, 15)])                     # a host tensor never reaches a launch


# ----------------------------------------------------------------------------- scan_frames end to end
def _ed(dtype):
    def make():
        m = GenConViTED(load_config(), init="empty")
        m.load_state_dict(synthetic_sd("ed"))
        return m.to("cuda").to(dtype).eval()
    return _cached(("ed", dtype), make)


def _vae(dtype):
    def make():
        m = GenConViTVAE(load_config(), init="empty")
        m.load_state_dict(synthetic_sd("vae"))
        return m.to("cuda").to(dtype).eval()
    return _cached(("vae", dtype), make)


def _scan_scene():
    """8 frames of 180 x 320; face 0 on every frame, drifting; face 1 seen on frames 1, 2, 5, 6: two frames to fill"""
    frames = torch.randint(0, 256, (8, 180, 320, 3), dtype=torch.uint8, generator=torch.Generator().manual_seed(21))
    boxes = [(f, 10 + f, 130 + 2 * f, 120 + f, 20 + f) for f in range(8)]
    boxes += [(1, 40, 300, 160, 200), (2, 42, 301, 161, 202), (5, 46, 306, 170, 205), (6, 47, 308, 172, 206)]
    return frames, boxes


KW = dict(detect_every=3, window=4, stride=2)        # explicit boxes: detect_every only sets the gap a track may bridge


def _per_crop_scores(frames, rows, model, nets, eps, max_batch):
    """mean over nets of sigmoid(model(preprocess_frame(crop_faces(...)))) per crop, float64 on the host, the crops taken
    in frame order in groups of max_batch like the scan does"""
    n = len(rows)
    order = sorted(range(n), key=lambda i: (rows[i][0], i))
    out = torch.empty((n, 2), dtype=torch.float64)
    dev = frames.cuda()
    for g in range(0, n, max_batch):
        ids = order[g:g + max_batch]
        df = pred_func.preprocess_frame(pred_func.crop_faces(dev, [rows[i] for i in ids]))
        logits = model(df) if eps is None else model(df, eps=eps[torch.as_tensor(ids, device="cuda")])
        out[ids] = torch.sigmoid(logits.double().cpu().reshape(nets, len(ids), 2)).mean(0)
    return out


def _check_verdict(what, got, want, pair, tol):
    """``got``, ``want``: (y, y_val) of the scan and of ``pred_vid``; ``pair``: the scan's own mean pair for those crops.
    Always asserted: the column of the mean pair that ``pred_vid``'s (y, y_val) reveals (m0 = y_val for y == 0,
    m1 = 1 - y_val for y == 1) agrees with the scan's within ``tol``.  The (y, y_val) themselves are compared too, always
    for fp32; under 16-bit storage only when the two columns are further apart than twice the storage bound — closer
    than that either y is a fair answer, and the skip is printed."""
    margin = abs(pair[0] - pair[1])
    col = want[1] if want[0] == 0 else 1.0 - want[1]
    print(f"{what}: scan {got} pair {pair}, pred_vid {want}, margin {margin:.3e}")
    assert abs(pair[want[0]] - col) <= tol, (pair, want)
    if tol > 1e-5 and margin <= 2 * tol:
        print(f"{what}: margin within {2 * tol:g}: y not compared")
        return
    assert got[0] == want[0] and abs(got[1] - want[1]) <= tol, (got, want)


@pytest.mark.parametrize("kind", ["ed fp32", "genconvit fp16"])
def test_scan_frames_on_the_device(kind):
    """fp32 ED: scores within 1e-5 of the per-crop path, verdicts equal to pred_vid's with |y_val| within 1e-5.  fp16
    ensemble (eps pinned): scores within 2e-3, the bound of fp16 storage used for the preprocessing above."""
    frames, boxes = _scan_scene()
    if kind == "ed fp32":
        model, nets, eps, tol = GenConViT.from_modules(_ed(torch.float32), None, net="ed"), 1, None, 1e-5
    else:
        model = GenConViT.from_modules(_ed(torch.float16), _vae(torch.float16), net="genconvit")
        nets, eps, tol = 2, synth.make_eps(14, name="scan").cuda(), 2e-3
    res = pred_func.scan_frames(frames.numpy(), model, boxes=boxes, max_batch=5, eps=eps, **KW)
    t0, t1 = res["tracks"]
    assert t0 == boxes[:8] and [b[0] for b in t1] == [1, 2, 3, 4, 5, 6] and res["track_offsets"] == [0, 8, 14]
    assert t1[2] == (3, 43, 303, 164, 203) and t1[3] == (4, 45, 304, 167, 204)            # floor(a + (b - a) k / 3 + 0.5)
    rows = res["boxes"]
    assert rows == t0 + t1 and res["frame_scores"].is_cuda and tuple(res["frame_scores"].shape) == (14, 2)
    want = _per_crop_scores(frames, rows, model, nets, eps, 5)
    err = (res["frame_scores"].cpu().double() - want).abs().max().item()
    print(f"\nscan_frames {kind}: max |frame_scores - per-crop path| = {err:.3e} (bound {tol:g})")
    assert err <= tol
    # windows: window_ranges over each track, offset by its first frame
    assert [w[:3] for w in res["windows"]] == [(t, tr[0][0] + lo, tr[0][0] + hi - 1) for t, tr in enumerate((t0, t1))
                                               for lo, hi in pred_func.window_ranges(len(tr), 4, 2)]
    assert [w[:3] for w in res["windows"]] == [(0, 0, 3), (0, 2, 5), (0, 4, 7), (1, 1, 4), (1, 3, 6)]
    fp = res["frame_scores"].cpu()
    for k, (t, first, last, y, y_val) in enumerate(res["windows"]):
        lo = res["track_offsets"][t] + first - res["tracks"][t][0][0]
        m = fp[lo:lo + last - first + 1].double().mean(0)
        assert (res["window_means"][k].cpu().double() - m).abs().max().item() <= 2e-6
        assert (y, y_val) == pred_func._verdict(res["window_means"][k].cpu())
    # verdicts: pred_vid on the same crops (eps pinned per crop)
    df = pred_func.preprocess_frame(pred_func.crop_faces(frames.cuda(), rows))

    def vid(lo, hi):
        m = model
        if eps is not None:
            class Pinned(torch.nn.Module):
                def __init__(self):
                    super().__init__()
                    self.g = model

                def forward(self, x):
                    return self.g(x, eps=eps[lo:hi])
            m = Pinned()
        return pred_func.pred_vid(df[lo:hi], m)
    _check_verdict(f"{kind} verdict", res["verdict"], vid(0, 14), fp.mean(0).tolist(), tol)
    for t in (0, 1):
        lo, hi = res["track_offsets"][t:t + 2]
        _check_verdict(f"{kind} track {t}", res["track_verdicts"][t], vid(lo, hi), fp[lo:hi].mean(0).tolist(), tol)
    # one group for everything: the same scores
    one = pred_func.scan_frames(frames.cuda(), model, boxes=boxes, max_batch=128, eps=eps, **KW)
    err = (one["frame_scores"] - res["frame_scores"]).abs().max().item()
    print(f"scan_frames {kind}: max |frame_scores, one group - groups of 5| = {err:.3e}")
    assert err <= tol and one["boxes"] == rows
    for seg in res["segments"]:
        assert any(w[0] == seg[0] and w[1] == seg[1] and w[3] == 0 for w in res["windows"])
