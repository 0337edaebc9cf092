"""gcv_cam_overlay on the MI355X against its CPU restatement (tests/overlayutil.py): torch.equal on every pixel of every
case, no tolerance and no excluded pixels.  Then ``pred_func.explain_frames`` end to end with synthetic weights: its verdict
is ``pred_vid_explain``'s for the same crops, and its overlays are the restatement applied to the maps ``model.explain``
returned for those crops, so the comparison does not depend on Grad-CAM numerics."""
import pytest
import torch

from genconvit_amd import _lib
from genconvit_amd.model import pred_func
from genconvit_amd.model.genconvit import normalize_cams
from tests import overlayutil as ou
from tests.conftest import synthetic_sd

pytestmark = pytest.mark.gpu
torch.set_grad_enabled(False)


def _frames(shape, seed):
    return torch.randint(0, 256, shape, dtype=torch.uint8, generator=torch.Generator().manual_seed(seed))


def _maps(n, mh, mw, seed):
    """Random maps in [0, 1] with exact zeros and ones among the cells."""
    g = torch.Generator().manual_seed(seed)
    m = torch.rand((n, mh, mw), generator=g)
    r = torch.rand((n, mh, mw), generator=g)
    return torch.where(r < 0.1, torch.zeros(()), torch.where(r > 0.9, torch.ones(()), m))


def _check(frames, boxes, maps, **kw):
    lut = kw.get("lut")
    dev_kw = dict(kw, lut=lut.cuda()) if lut is not None else kw
    got = _lib.cam_overlay(frames.cuda(), boxes, maps.cuda(), **dev_kw).cpu()
    want = ou.overlay_ref(frames, boxes, maps, kw.get("alpha", 0.5), kw.get("weighted", True), lut)
    bad = (got != want).any(-1)
    assert torch.equal(got, want), f"{int(bad.sum())} of {bad.numel()} pixels differ, first at {bad.nonzero()[:4].tolist()}"
    return got


def _random_boxes(nf, H, W, n, seed, min_side=1):
    g = torch.Generator().manual_seed(seed)
    r = lambda lo, hi: int(torch.randint(lo, hi + 1, (1,), generator=g))
    boxes = []
    for _ in range(n):
        h, w = r(min_side, H), r(min_side, W)
        top, left = r(0, H - h), r(0, W - w)
        boxes.append((r(0, nf - 1), top, left + w, top + h, left))
    return boxes


# ----------------------------------------------------------------------------- the kernel
@pytest.mark.parametrize("weighted", [True, False], ids=["weighted", "flat"])
@pytest.mark.parametrize("alpha", [0.0, 0.5, 1.0])
@pytest.mark.parametrize("m", [1, 3, 7, 14, 224])
def test_overlay_map_sizes_alpha_and_weighting(m, alpha, weighted):
    """Boxes smaller and larger than the map, 1-pixel boxes, boxes on each frame edge and a whole-frame box, on an odd frame
    width; frame 2 has no box."""
    H, W = 250, 333
    frames = _frames((4, H, W, 3), 10 + m)
    boxes = [(0, 0, W, H, 0),                     # whole frame
             (1, 0, 120, 90, 0),                  # top-left corner
             (1, 0, W, 5, W - 3),                 # top-right corner, 3 wide
             (1, H - 40, 61, H, 0),               # bottom-left
             (1, H - 229, W, H, W - 230),         # bottom-right, larger than every map
             (1, 100, 101, 101, 100),             # one pixel
             (3, 17, 19, 200, 18),                # one column
             (3, 249, 300, 250, 1),               # one row, the last of the frame
             (3, 30, 37, 33, 30),                 # smaller than most maps
             (3, 40, 280, 47, 273)]               # 7 x 7
    _check(frames, boxes, _maps(len(boxes), m, m, 20 + m), alpha=alpha, weighted=weighted)


def test_overlay_non_square_maps_and_other_alphas():
    frames = _frames((2, 97, 131, 3), 1)
    boxes = _random_boxes(2, 97, 131, 6, 2)
    for (mh, mw), alpha in (((7, 14), 0.3), ((14, 3), 0.77), ((1, 224), 0.999), ((5, 1), 0.004)):
        for weighted in (True, False):
            _check(frames, boxes, _maps(6, mh, mw, mh), alpha=alpha, weighted=weighted)


@pytest.mark.parametrize("W", [641, 1, 2, 3, 5, 1023, 1024, 1366])
def test_overlay_odd_widths_and_piece_edges(W):
    """Rows of 3 W bytes start anywhere in a thread's 12-byte piece; box edges fall inside pieces; the tensor ends inside
    one."""
    H, nf = (7, 5) if W > 5 else (9, 3)
    frames = _frames((nf, H, W, 3), W)
    boxes = _random_boxes(nf, H, W, 12, W + 1)
    boxes += [(0, 0, min(W, left + 1 + k), H, left) for k, left in enumerate(range(min(W, 9)))]      # every start phase
    boxes.append((nf - 1, H - 1, W, H, W - 1))                                                      # the very last pixel
    _check(frames, boxes, _maps(len(boxes), 7, 7, W + 2))


def test_overlay_full_hd_clip():
    """15 frames of 1080 x 1920, one face a frame and a second, overlapping one on two of them."""
    frames = _frames((15, 1080, 1920, 3), 3)
    boxes = [(f, 100 + 31 * f, 700 + 40 * f + 380 + f, 100 + 31 * f + 420 - f, 700 + 40 * f) for f in range(15)]
    boxes += [(4, 300, 1100, 700, 800), (9, 0, 1920, 1080, 1500)]
    _check(frames, boxes, _maps(len(boxes), 7, 7, 4))
    _check(frames, boxes, _maps(len(boxes), 14, 14, 5), alpha=1.0, weighted=False)


def test_overlay_overlapping_and_nested_boxes_in_row_order():
    frames = _frames((3, 120, 161, 3), 6)
    boxes = [(0, 10, 100, 100, 10), (0, 30, 80, 80, 30), (0, 40, 70, 70, 40),      # nested three deep
             (1, 5, 90, 60, 5), (1, 40, 150, 110, 60), (1, 20, 75, 119, 55),        # chained overlaps
             (0, 50, 161, 90, 60), (1, 5, 90, 60, 5),                               # back to earlier frames; a repeated box
             (2, 0, 161, 120, 0), (2, 0, 161, 120, 0)]                              # the whole frame twice
    maps = _maps(len(boxes), 7, 7, 7)
    for alpha, weighted in ((0.5, True), (0.5, False), (1.0, False)):
        got = _check(frames, boxes, maps, alpha=alpha, weighted=weighted)
    # row order matters: the reverse order draws something else, and that too is the restatement's
    rev = _check(frames, boxes[::-1], maps.flip(0), alpha=1.0, weighted=False)
    assert not torch.equal(rev, got)


def test_overlay_many_boxes_more_than_one_scan_round():
    """More boxes than the 256 a block tests at a time, scattered over few small frames."""
    frames = _frames((3, 64, 75, 3), 8)
    boxes = _random_boxes(3, 64, 75, 700, 9, min_side=1)
    _check(frames, boxes, _maps(700, 3, 3, 10), alpha=0.6, weighted=False)


def test_overlay_tiny_frames_several_in_one_block():
    frames = _frames((300, 5, 7, 3), 11)
    boxes = _random_boxes(300, 5, 7, 200, 12)
    _check(frames, boxes, _maps(200, 7, 7, 13))


def test_overlay_no_boxes_copies_the_frames():
    frames = _frames((2, 33, 47, 3), 14)
    got = _lib.cam_overlay(frames.cuda(), [], torch.empty((0, 7, 7), device="cuda"))
    assert torch.equal(got.cpu(), frames)
    fd = frames.cuda()
    assert _lib.cam_overlay(fd, [], torch.empty((0, 7, 7), device="cuda"), out=fd) is fd
    assert torch.equal(fd.cpu(), frames)
    # boxes on some frames only: the others come through unchanged
    got = _check(frames, [(1, 3, 40, 30, 4)], _maps(1, 7, 7, 15))
    assert torch.equal(got[0], frames[0])


def test_overlay_callers_lut():
    frames = _frames((2, 60, 81, 3), 16)
    boxes = _random_boxes(2, 60, 81, 5, 17)
    _check(frames, boxes, _maps(5, 14, 14, 18), alpha=0.8, weighted=False, lut=_frames((256, 3), 19))
    _check(frames, boxes, _maps(5, 14, 14, 18), alpha=0.8, weighted=True, lut=_frames((256, 3), 20))


def test_overlay_non_contiguous_frames():
    big = _frames((3, 70, 120, 3), 21)
    view = big[:, 5:66, 10:101]                                   # (3, 61, 91, 3), strided
    assert not view.is_contiguous()
    boxes = _random_boxes(3, 61, 91, 6, 22)
    maps = _maps(6, 7, 7, 23)
    got = _lib.cam_overlay(big.cuda()[:, 5:66, 10:101], boxes, maps.cuda())
    assert torch.equal(got.cpu(), ou.overlay_ref(view, boxes, maps))
    # a contiguous tensor that does not start on a 4-byte boundary (the byte-wise arm)
    flat = _frames((1 + 2 * 31 * 45 * 3,), 24).cuda()
    odd = flat[1:].view(2, 31, 45, 3)
    assert odd.is_contiguous() and odd.data_ptr() % 4 != 0
    boxes = _random_boxes(2, 31, 45, 5, 25)
    out = torch.empty_like(flat)[1:].view(2, 31, 45, 3)
    got = _lib.cam_overlay(odd, boxes, maps[:5].cuda(), out=out)
    assert got is out and torch.equal(got.cpu(), ou.overlay_ref(odd.cpu(), boxes, maps[:5]))


def test_overlay_out_given_and_in_place():
    frames = _frames((3, 90, 127, 3), 26)
    boxes = _random_boxes(3, 90, 127, 8, 27) + [(0, 0, 127, 90, 0)]
    maps = _maps(9, 14, 14, 28)
    want = ou.overlay_ref(frames, boxes, maps)
    fd = frames.cuda()
    out = torch.full_like(fd, 7)
    assert _lib.cam_overlay(fd, boxes, maps.cuda(), out=out) is out
    assert torch.equal(out.cpu(), want) and torch.equal(fd.cpu(), frames)
    assert _lib.cam_overlay(fd, boxes, maps.cuda(), out=fd) is fd             # in place
    assert torch.equal(fd.cpu(), want)
    with pytest.raises(_lib.GenConViTHipError, match="out"):
        _lib.cam_overlay(fd, boxes, maps.cuda(), out=torch.empty((3, 90, 128, 3), dtype=torch.uint8, device="cuda"))
    with pytest.raises(_lib.GenConViTHipError, match="maps"):
        _lib.cam_overlay(fd, boxes, maps)                                      # maps on the host


def test_overlay_128_crops_with_whole_frame_boxes():
    """Overlaying a batch of 224 x 224 crops is one whole-frame box per crop."""
    frames = _frames((128, 224, 224, 3), 29)
    boxes = [(i, 0, 224, 224, 0) for i in range(128)]
    _check(frames, boxes, _maps(128, 14, 14, 30))
    _check(frames, boxes, _maps(128, 7, 7, 31), alpha=0.7, weighted=False)
    _check(frames[:16], boxes[:16], _maps(16, 224, 224, 32))


def test_overlay_half_precision_maps_are_taken_as_fp32():
    frames = _frames((1, 50, 50, 3), 33)
    maps = _maps(1, 7, 7, 34).half()
    got = _lib.cam_overlay(frames.cuda(), [(0, 5, 45, 45, 5)], maps.cuda())
    assert torch.equal(got.cpu(), ou.overlay_ref(frames, [(0, 5, 45, 45, 5)], maps.float()))


# ----------------------------------------------------------------------------- explain_frames end to end
_MODELS = {}


def _model(net):
    from genconvit_amd.model.config import load_config
    from genconvit_amd.model.genconvit import GenConViT
    from genconvit_amd.model.genconvit_ed import GenConViTED
    from genconvit_amd.model.genconvit_vae import GenConViTVAE
    if net not in _MODELS:
        ed = GenConViTED(load_config(), init="empty")
        ed.load_state_dict(synthetic_sd("ed"))
        vae = None
        if net != "ed":
            vae = GenConViTVAE(load_config(), init="empty")
            vae.load_state_dict(synthetic_sd("vae"), strict=False)
            vae.keep_kl_weights = False
            vae = vae.cuda().eval()
        _MODELS[net] = GenConViT.from_modules(ed.cuda().eval(), vae, net=net, fp16=True)
    return _MODELS[net]


_E2E_BOXES = [(0, 20, 200, 180, 40), (0, 100, 400, 290, 150), (2, 0, 417, 300, 0), (3, 33, 130, 97, 81), (4, 150, 300, 299, 1)]


def _want_maps(net, cams, which):
    ed = lambda: normalize_cams(cams["ed"][:, 1])
    vae = lambda: normalize_cams(cams["vae"])
    if net == "ed":
        return ed()
    return {"ed": ed, "vae": vae, "mean": lambda: (ed() + vae()) / 2}[which]()


@pytest.mark.parametrize("which", ["mean", "ed", "vae"])
@pytest.mark.parametrize("layer", ["s3", "s2"])
@pytest.mark.parametrize("net", ["ed", "genconvit"])
def test_explain_frames_end_to_end(net, layer, which):
    model = _model(net)
    frames = _frames((5, 300, 417, 3), 40)                       # two faces on frame 0, none on frame 1
    n = len(_E2E_BOXES)
    eps = torch.randn((n, 12544), device="cuda", generator=torch.Generator("cuda").manual_seed(41))
    calls = []

    def locate(fr):
        calls.append(len(fr))
        return list(_E2E_BOXES)

    (y, y_val), overlays, boxes = pred_func.explain_frames(frames.numpy(), model, locate=locate, eps=eps, layer=layer,
                                                           which=which, alpha=0.6)
    assert calls == [5] and boxes == _E2E_BOXES
    assert overlays.is_cuda and overlays.dtype == torch.uint8 and overlays.shape == frames.shape
    # the same crops through the existing entries
    df = pred_func.preprocess_frame(pred_func.crop_faces(frames.numpy(), boxes).cpu().numpy())
    if net != "ed":
        model.model_vae.set_generator(torch.Generator("cuda").manual_seed(41))     # pred_vid_explain draws eps itself
    try:
        want_verdict, _ = pred_func.pred_vid_explain(df, model, layer=layer)
    finally:
        if net != "ed":
            model.model_vae.set_generator(None)
    assert (y, y_val) == want_verdict
    _, cams = model.explain(df, eps=eps, upsample=False, layer=layer)
    side = 7 if layer == "s3" else 14
    maps = _want_maps(net, cams, which)
    assert maps.shape == (n, side, side)
    want = ou.overlay_ref(frames, boxes, maps.cpu(), 0.6, True)
    assert torch.equal(overlays.cpu(), want)
    assert torch.equal(want[1], frames[1]) and not torch.equal(want[0], frames[0])


def test_explain_frames_boxes_given_tensor_frames_target_and_reference_dtype():
    """``boxes=`` instead of a detector, frames as a device tensor, an explicit target, a flat blend with a caller's LUT, and
    the verdict under ``reference_logits_dtype``."""
    model = _model("genconvit")
    frames = _frames((3, 240, 320, 3), 42)
    boxes = [(0, 10, 200, 230, 30), (1, 0, 320, 240, 0), (2, 50, 101, 99, 50), (2, 60, 300, 200, 90)]   # cut at 3 rows
    eps = torch.randn((3, 12544), device="cuda", generator=torch.Generator("cuda").manual_seed(43))
    lut = _frames((256, 3), 44)
    target = torch.tensor([1, 0, 1], dtype=torch.int32)
    model.reference_logits_dtype = True
    try:
        (y, y_val), overlays, used = pred_func.explain_frames(frames.cuda(), model, boxes=boxes, eps=eps, target=target,
                                                              layer="s2", which="vae", alpha=1.0, weighted=False,
                                                              lut=lut.cuda())
        assert used == boxes[:3]
        df = pred_func.preprocess_frame(pred_func.crop_faces(frames, used))
        logits, cams = model.explain(df, eps=eps, target=target, upsample=False, layer="s2")
        assert (y, y_val) == pred_func.max_prediction_value(torch.sigmoid(logits.half().squeeze()))
    finally:
        model.reference_logits_dtype = False
    want = ou.overlay_ref(frames, used, normalize_cams(cams["vae"]).cpu(), 1.0, False, lut)
    assert torch.equal(overlays.cpu(), want)


def test_explain_frames_without_a_face():
    frames = _frames((2, 60, 80, 3), 45)
    (y, y_val), overlays, boxes = pred_func.explain_frames(frames.numpy(), _model("ed"), locate=lambda fr: [])
    assert (y, y_val) == (None, None) and boxes == []
    assert overlays.is_cuda and torch.equal(overlays.cpu(), frames)
