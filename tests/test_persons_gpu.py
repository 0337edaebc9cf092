"""``gcv_face_signature`` and ``gcv_sig_link`` on the MI355X, bit for bit against their CPU restatements
(tests/personutil.py: ``torch.equal``, no tolerance — the arithmetic is integer), their guards and refusals through the C
entries, and ``pred_func.scan_frames(persons=True)`` end to end with synthetic weights.  The inputs are
``personutil.signature_case`` and ``personutil.link_cases``: tests/test_persons_sensitivity_cpu.py shows, without a GPU,
that kernels with a planted defect could not pass on them."""
import numpy as np
import pytest
import torch

from genconvit_amd import _lib
from genconvit_amd.model import pred_func
from genconvit_amd.model.genconvit import GenConViT
from tests import personutil as pu

pytestmark = pytest.mark.gpu
torch.set_grad_enabled(False)


def _assert_signatures(frames, boxes, dev=None):
    dev = torch.as_tensor(frames).cuda() if dev is None else dev
    got = _lib.face_signature(dev, boxes)
    assert got.is_cuda and got.dtype == torch.uint8 and tuple(got.shape) == (len(boxes), 384)
    want = torch.as_tensor(pu.face_signature_ref(frames, boxes))
    if not torch.equal(got.cpu(), want):
        bad = (got.cpu() != want).any(1).nonzero().flatten().tolist()
        k = (got[bad[0]].cpu() != want[bad[0]]).nonzero().flatten().tolist()
        raise AssertionError(f"boxes {bad} differ; first: box {boxes[bad[0]]} bytes {k[:8]} got "
                             f"{got[bad[0]].cpu()[k[:8]].tolist()} want {want[bad[0]][k[:8]].tolist()}")
    return got


# ----------------------------------------------------------------------------- signatures
def test_face_signature_boxes_of_every_kind():
    frames, boxes = pu.signature_case()
    got = _assert_signatures(frames, boxes).cpu()
    assert got[10, :256].eq(128).all() and got[11, :256].eq(128).all()                      # the flat frame: A = 0
    assert got[12, :256].max() == 255 and got[13, :256].min() == 0                          # the stripes clamp


def test_face_signature_on_an_unaligned_slice_and_without_boxes():
    """frames of 37 x 53 taken as frames[1:]: the base pointer is 5 883 bytes into the allocation"""
    frames = np.random.default_rng(31).integers(0, 256, (4, 37, 53, 3), dtype=np.uint8)
    dev = torch.as_tensor(frames).cuda()[1:]
    assert dev.data_ptr() % 2 == 1 and dev.is_contiguous()
    boxes = [(f, 0, 53, 37, 0) for f in range(3)] + [(0, 0, 17, 16, 0), (2, 21, 53, 37, 37), (1, 9, 40, 30, 12)]
    _assert_signatures(frames[1:], boxes, dev=dev)
    none = _lib.face_signature(dev, [])
    assert tuple(none.shape) == (0, 384) and none.dtype == torch.uint8 and none.is_cuda


def test_face_signature_guard_and_refusals_through_the_c_entry():
    frames, boxes = pu.signature_case()
    dev = torch.as_tensor(frames).cuda()
    for box in ((5, 0, 40, 40, 0), (0, 0, 129, 40, 0), (0, -1, 40, 40, 0), (0, 0, 15, 40, 0)):
        with pytest.raises(_lib.GenConViTHipError):
            _lib.face_signature(dev, [boxes[0], box])
    with pytest.raises(_lib.GenConViTHipError):
        _lib.face_signature(dev.cpu(), boxes)
    lib = _lib.load()
    rows = [boxes[0], (5, *boxes[1][1:]), boxes[2], (0, 10, 35, 60, 20), (0, 0, 400, 40, 0)]  # frame 5 of 5; 15 wide; outside
    bd = torch.as_tensor(rows, dtype=torch.int32).cuda()
    out = torch.full((5, 384), 7, dtype=torch.uint8, device="cuda")
    stream = _lib.current_stream_ptr(dev.device)

    def call(nf=5, h=96, w=128, n=5, fp=dev.data_ptr(), bp=bd.data_ptr(), op=out.data_ptr()):
        return lib.gcv_face_signature(fp, nf, h, w, bp, n, op, stream)
    for kw in (dict(nf=0), dict(h=0), dict(w=-1), dict(h=1 << 15, w=(1 << 13) + 1), dict(fp=None), dict(bp=None), dict(op=None),
               dict(n=-1)):
        assert call(**kw) != 0 and _lib.last_error(), kw
    assert call(n=0) == 0 and call(n=0, fp=None, bp=None, op=None) == 0
    torch.cuda.synchronize()
    assert bool((out == 7).all())                                                           # nothing was launched so far
    # rows the binding would refuse give 384 zeros and read nothing; the good rows beside them are served
    assert call() == 0
    want = torch.as_tensor(pu.face_signature_ref(frames, [boxes[0], boxes[2]]))
    got = out.cpu()
    assert torch.equal(got[[0, 2]], want) and not got[[1, 3, 4]].any()


# ----------------------------------------------------------------------------- link
@pytest.mark.parametrize("case", pu.link_cases(), ids=lambda c: c[0])
def test_sig_link(case):
    name, sig, owner, T = case
    got = _lib.sig_link(torch.as_tensor(sig).cuda(), owner, T)
    assert got.is_cuda and got.dtype == torch.int64 and tuple(got.shape) == (T, T)
    want = torch.as_tensor(pu.sig_link_ref(sig, owner, T))
    assert torch.equal(got.cpu(), want), (name, got.cpu().tolist(), want.tolist())
    assert torch.equal(got, got.T) and bool((got.diagonal() == pu.NONE).all())
    if name == "equal rows":
        assert got[0, 1].item() == 0
    if name == "0 against 255":
        assert got[0, 1].item() == 97920
    if name == "empty track":
        assert bool((got[2] == pu.NONE).all())


def test_sig_link_without_rows_and_refusals_through_the_c_entry():
    sig = torch.as_tensor(pu.link_cases()[1][1]).cuda()                                      # 63 rows
    assert _lib.sig_link(sig[:0], [], 3).tolist() == [[pu.NONE] * 3] * 3
    assert tuple(_lib.sig_link(sig, [-1] * 63, 0).shape) == (0, 0)
    with pytest.raises(_lib.GenConViTHipError):
        _lib.sig_link(sig, [3] * 63, 3)
    with pytest.raises(_lib.GenConViTHipError):
        _lib.sig_link(sig.cpu(), [0] * 63, 3)
    lib = _lib.load()
    owner = torch.as_tensor([i % 2 for i in range(63)], dtype=torch.int32).cuda()
    out = torch.full((2, 2), 7, dtype=torch.int32, device="cuda")
    stream = _lib.current_stream_ptr(sig.device)

    def call(n=63, T=2, sp=sig.data_ptr(), wp=owner.data_ptr(), op=out.data_ptr()):
        return lib.gcv_sig_link(sp, wp, n, T, op, stream)
    for kw in (dict(n=-1), dict(n=65537), dict(T=-1), dict(T=4097), dict(sp=None), dict(wp=None), dict(op=None),
               dict(sp=sig.data_ptr() + 4)):
        assert call(**kw) != 0 and _lib.last_error(), kw
    assert call(n=0) == 0 and call(T=0) == 0 and call(n=0, sp=None, wp=None, op=None) == 0
    torch.cuda.synchronize()
    assert bool((out == 7).all())                                                           # nothing was written so far
    # an owner outside [0, T), which the binding refuses, takes no part and writes nowhere
    owner[5], owner[6] = 2, -9
    assert call() == 0
    o = owner.cpu().tolist()
    want = pu.sig_link_ref(sig, [v if 0 <= v < 2 else -1 for v in o], 2)
    assert (out.cpu().to(torch.int64) & pu.NONE).tolist() == want.tolist()


# ----------------------------------------------------------------------------- scan_frames(persons=True) end to end
def _model():
    """the fp32 ED of tests/test_scan_gpu.py: the same cached network, built once per session"""
    from tests.test_scan_gpu import _ed
    return GenConViT.from_modules(_ed(torch.float32), None, net="ed")


def test_scan_frames_persons_on_the_device():
    """four shots cutting between two synthetic identities: the distances are the restatement's, the two persons are found,
    a person of one track has that track's verdict and mean (the same <= 16 fp32 values in [0, 1] summed in another
    order: below 16 * 2^-24 < 1e-6), and every other key is what the scan without ``persons`` gives"""
    frames, det, cuts = pu.interview()
    model = _model()
    kw = dict(boxes=det, window=3, cuts=cuts, max_batch=8)
    plain = pred_func.scan_frames(frames, model, **kw)
    res = pred_func.scan_frames(frames, model, persons=True, **kw)
    assert sorted(res) == sorted(list(plain) + ["persons"])
    for key, val in plain.items():
        assert torch.equal(res[key], val) if torch.is_tensor(val) else res[key] == val, key
    p = res["persons"]
    want = pu.sig_link_ref(pu.face_signature_ref(frames, res["boxes"]), [t for t in range(4) for _ in range(4)], 4)
    assert p["distance"].dtype == np.int64 and (p["distance"] == want).all()
    assert p["tracks"] == [[0, 2], [1, 3]] and p["of_track"] == [0, 1, 0, 1] and p["measured"].all()
    fp = res["frame_scores"].double().cpu()
    for k, rows in enumerate(([0, 1, 2, 3, 8, 9, 10, 11], [4, 5, 6, 7, 12, 13, 14, 15])):
        assert (p["means"][k].double().cpu() - fp[rows].mean(0)).abs().max().item() <= 1e-6
        assert p["verdicts"][k] == pred_func._verdict(p["means"][k].cpu())
    # from frames already on the device, and with nothing linked: every person is one track
    # (window = 4 = a track's length: window t is the whole of track t, and window_means[t] the track's mean pair)
    alone = pred_func.scan_frames(torch.as_tensor(frames).cuda(), model, persons=True, person_args=dict(link_max=0),
                                  **{**kw, "window": 4})
    q = alone["persons"]
    assert (q["distance"] == want).all() and q["tracks"] == [[0], [1], [2], [3]]
    assert q["verdicts"] == alone["track_verdicts"]
    assert [w[:3] for w in alone["windows"]] == [(t, 4 * t, 4 * t + 3) for t in range(4)]
    err = (q["means"].double() - alone["window_means"].double()).abs().max().item()
    print(f"\nscan_frames(persons=True): max |mean of a one-track person - the track's mean| = {err:.3e} (bound 1e-06)")
    assert err <= 1e-6
