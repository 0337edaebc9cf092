"""``gcv_face_quality`` on the MI355X, bit for bit against its CPU restatement (tests/qualityutil.py: all eight columns,
``torch.equal``, no tolerance — the arithmetic is integer), its guard and its refusals through the C entry, and
``pred_func.scan_frames(quality=True)`` end to end with synthetic weights."""
import numpy as np
import pytest
import torch

from genconvit_amd import _lib
from genconvit_amd.model import pred_func
from genconvit_amd.model.genconvit import GenConViT
from tests import qualityutil as qu

pytestmark = pytest.mark.gpu
torch.set_grad_enabled(False)

_CACHE = {}


def _cached(key, make):
    if key not in _CACHE:
        _CACHE[key] = make()
    return _CACHE[key]


def _assert_same(frames, boxes, grid, dev=None):
    """``frames``: the host array the restatement reads; ``dev``: the same frames on the device (uploaded if not given)"""
    dev = torch.as_tensor(frames).cuda() if dev is None else dev
    got = _lib.face_quality(dev, boxes, grid=grid)
    assert got.is_cuda and got.dtype == torch.int64 and tuple(got.shape) == (len(boxes), 8)
    want = torch.as_tensor(qu.face_quality_ref(frames, boxes, grid))
    if not torch.equal(got.cpu(), want):
        bad = (got.cpu() != want).any(1).nonzero().flatten().tolist()
        raise AssertionError(f"grid {grid}: boxes {bad} differ; first: box {boxes[bad[0]]} got {got[bad[0]].tolist()} want "
                             f"{want[bad[0]].tolist()}")
    return got.cpu()


def _fuzz(grid):
    """qualityutil.fuzz_boxes, made once per grid"""
    return _cached(("fuzz", grid), lambda: qu.fuzz_boxes(grid))


@pytest.mark.parametrize("grid", [16, 32])
def test_face_quality_random_boxes(grid):
    frames, boxes = _fuzz(grid)
    assert len(boxes) == 48 and {0} == {min(b[1] for b in boxes), min(b[4] for b in boxes)}
    assert max(b[3] for b in boxes) == 120 and max(b[2] for b in boxes) == 160
    got = _assert_same(frames, boxes, grid)
    assert bool((got[:, 0] == grid).all())


@pytest.mark.parametrize("grid", [16, 32, 64])
def test_face_quality_edge_boxes(grid):
    """boxes one pixel over the grid in one direction, the whole frame, and a box in each corner of the frame"""
    frames, _ = _fuzz(16)
    _assert_same(frames, qu.edge_boxes(grid), grid)


@pytest.mark.parametrize("grid", [16, 32, 64])
def test_face_quality_flat_black_and_white_frames(grid):
    frames, boxes = qu.flat_case()                                                         # Y = 124, black, white
    got = _assert_same(frames, boxes, grid)
    n = grid * grid
    assert got[:3].tolist() == [[grid, n * 124, n * 124 * 124, 0, 0, 0, 0, 0], [grid, 0, 0, 0, 0, 0, n, 0],
                                [grid, n * 255, n * 255 * 255, 0, 0, 0, 0, n]]


def test_face_quality_on_an_unaligned_slice():
    """frames of 37 x 53 taken as frames[1:]: the base pointer is 5 883 bytes into the allocation"""
    frames, boxes = qu.unaligned_case()
    dev = torch.as_tensor(frames).cuda()[1:]
    assert dev.data_ptr() % 2 == 1 and dev.is_contiguous()
    _assert_same(frames[1:], boxes, 16, dev=dev)


def test_face_quality_largest_configuration():
    """grid 64, every lane 16 cells; 2 frames of 300 x 400 with the whole frame as a box: the most pixels a cell holds here"""
    frames, boxes = qu.largest_case()
    _assert_same(frames, boxes, 64)


@pytest.mark.parametrize("grid", [16, 32, 64])
def test_face_quality_checkerboard_reaches_the_largest_sums(grid):
    """squares of 2 x 2 pixels that alternate between 0 and 255, the whole frame as the box: every interior Laplacian is
    +-1020.  At grid 64 a lane's 16 cells add 16 * 1020^2, a wave 16 * 62 * 1020^2 (both just inside the 24 and 31 bits the
    kernel counts on), and L2 = 3 999 297 600 is more than a signed 32-bit total holds."""
    frames, boxes = qu.checkerboard(grid, 2)
    got = _assert_same(frames, boxes, grid)
    n = grid * grid
    assert got.tolist() == [[grid, n // 2 * 255, n // 2 * 255 ** 2, (grid - 2) ** 2 * 1020 ** 2, grid * (grid - 1) * 255 ** 2,
                             grid * (grid - 1) * 255 ** 2, n // 2, n // 2]]
    if grid == 64:
        assert got.tolist() == [qu.CHECKERBOARD_64] and qu.CHECKERBOARD_64[3] == 3999297600 > 2 ** 31


def test_face_quality_guard_and_refusals_through_the_c_entry():
    frames, boxes = _fuzz(16)
    dev = torch.as_tensor(frames).cuda()
    none = _lib.face_quality(dev, [], grid=16)
    assert tuple(none.shape) == (0, 8) and none.dtype == torch.int64 and none.is_cuda
    for grid in (8, 48, 128):
        with pytest.raises(_lib.GenConViTHipError):
            _lib.face_quality(dev, boxes, grid=grid)
    for box in ((3, 0, 40, 40, 0), (0, 0, 161, 40, 0), (0, -1, 40, 40, 0), (0, 0, 15, 40, 0)):
        with pytest.raises(_lib.GenConViTHipError):
            _lib.face_quality(dev, [boxes[0], box], grid=16)
    with pytest.raises(_lib.GenConViTHipError):
        _lib.face_quality(dev.cpu(), boxes, grid=16)                          # a host tensor never reaches a launch
    # the launcher's own checks, through the C ABI: refused with a reason, and nothing is launched
    lib = _lib.load()
    rows = [boxes[0], boxes[1], boxes[2], boxes[3], boxes[4]]
    bd = torch.as_tensor(rows, dtype=torch.int32).cuda()
    out = torch.full((5, 8), -7, dtype=torch.int64, device="cuda")
    stream = _lib.current_stream_ptr(dev.device)

    def call(nf=3, h=120, w=160, n=5, grid=16, fp=dev.data_ptr(), bp=bd.data_ptr(), op=out.data_ptr()):
        return lib.gcv_face_quality(fp, nf, h, w, bp, n, grid, op, stream)
    for kw in (dict(grid=8), dict(grid=0), dict(grid=65), dict(grid=-16), dict(nf=0), dict(h=0), dict(w=-1),
               dict(h=1 << 16, w=(1 << 14) + 1), dict(fp=None), dict(bp=None), dict(op=None)):
        assert call(**kw) != 0 and _lib.last_error(), kw
        with pytest.raises(_lib.GenConViTHipError):
            _lib.check(call(**kw), "gcv_face_quality")
    assert call(n=0) == 0 and call(n=0, fp=None, bp=None, op=None) == 0
    torch.cuda.synchronize()
    assert bool((out == -7).all())                                            # nothing was launched so far
    # rows the binding would refuse give eight zeros and read nothing; the good rows beside them are served
    rows[1] = (3, *boxes[1][1:])                                              # frame 3 of 3
    rows[3] = (*boxes[3][:2], 400, *boxes[3][3:])                             # right = 400 in a frame of 160
    bd.copy_(torch.as_tensor(rows, dtype=torch.int32))
    assert call() == 0
    want = qu.face_quality_ref(frames, [boxes[0], boxes[2], boxes[4]], 16).tolist()
    assert out.cpu().tolist() == [want[0], [0] * 8, want[1], [0] * 8, want[2]]
    small = [(0, 10, 60, 25, 20), (0, 10, 35, 60, 20), boxes[0], boxes[1], boxes[2]]      # 15 high, 15 wide: below the grid
    bd.copy_(torch.as_tensor(small, dtype=torch.int32))
    out.fill_(-7)
    assert call() == 0
    assert out.cpu().tolist() == [[0] * 8, [0] * 8] + qu.face_quality_ref(frames, boxes[:3], 16).tolist()
    # and a valid call after all that is correct
    _assert_same(frames, boxes, 16, dev=dev)


# ----------------------------------------------------------------------------- scan_frames(quality=True) end to end
def _model():
    """the fp32 ED of tests/test_scan_gpu.py: the same cached network, built once per session"""
    from tests.test_scan_gpu import _ed
    return GenConViT.from_modules(_ed(torch.float32), None, net="ed")


def test_scan_frames_quality_on_the_device():
    """two static faces over 10 frames, one of them blurred in three: the measures are the restatement's, the dropped rows
    the planted ones, and the scores of the kept rows those of the model on the crops of the kept boxes — within 1e-5, the
    bound of tests/test_scan_gpu.py for the fp32 ED against the per-crop path"""
    frames, det = qu.gated_video()
    dev = torch.as_tensor(frames).cuda()
    model = _model()
    kw = dict(boxes=det, window=3, quality=True, quality_args=dict(grid=16))
    res = pred_func.scan_frames(dev, model, **kw)
    q = res["quality"]
    before = [(f, *qu.FACE_A) for f in range(10)] + [(f, *qu.FACE_B) for f in range(10)]
    assert q["boxes"] == before and q["measured"].all()
    assert (q["raw"] == qu.face_quality_ref(frames, before, 16)).all()
    assert np.nonzero(~q["kept"])[0].tolist() == list(qu.PLANTED) and q["track_map"] == [0, 1]
    rows = [b for b, k in zip(before, q["kept"]) if k]
    assert res["boxes"] == rows and res["track_offsets"] == [0, 7, 17] and tuple(res["frame_scores"].shape) == (17, 2)
    want = torch.sigmoid(model(_lib.face_crop_preprocess(dev, rows, dtype=torch.float32)).double().cpu().reshape(1, 17, 2)).mean(0)
    err = (res["frame_scores"].cpu().double() - want).abs().max().item()
    print(f"\nscan_frames(quality=True): max |frame_scores - model(face_crop_preprocess(kept boxes))| = {err:.3e} (bound 1e-05)")
    assert err <= 1e-5
    # the same scan from host frames, uploaded in groups of two
    host = pred_func.scan_frames(frames, model, max_batch=2, **kw)
    assert sorted(host["quality"]) == sorted(q)
    for key, val in q.items():
        same = np.array_equal(host["quality"][key], val, equal_nan=True) if isinstance(val, np.ndarray) and \
            val.dtype == np.float64 else np.array_equal(host["quality"][key], val)
        assert same, key
    assert host["boxes"] == res["boxes"]
    assert (host["frame_scores"] - res["frame_scores"]).abs().max().item() <= 1e-5
