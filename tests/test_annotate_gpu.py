"""gcv_scan_annotate on the MI355X against its CPU restatement (tests/annotateutil.py): torch.equal on every pixel of every
case, no tolerance and no excluded pixels — the cases are the ones tests/test_annotate_sensitivity_cpu.py audits.  Then
``pred_func.render_scan`` end to end with synthetic weights: its frames are the restatement applied, after
``_lib.cam_overlay`` with the maps ``model.explain`` returns for the same crops and noise, to marks and a timeline this file
builds from ``res`` itself, so the comparison does not depend on Grad-CAM numerics."""
import pytest
import torch

from genconvit_amd import _lib, synth
from genconvit_amd.model import pred_func
from genconvit_amd.model.config import load_config
from genconvit_amd.model.genconvit import GenConViT
from genconvit_amd.model.genconvit_ed import GenConViTED
from genconvit_amd.model.genconvit_vae import GenConViTVAE
from tests import annotateutil as au
from tests.conftest import synthetic_sd

pytestmark = pytest.mark.gpu
torch.set_grad_enabled(False)

NAMES = list(au.cases()) + ["full hd"]
_CASES = {}


def _case(name):
    if not _CASES:
        _CASES.update(au.cases(full_hd=True))
    return _CASES[name]


def _same(got, want):
    bad = (got != want).any(-1)
    assert torch.equal(got, want), f"{int(bad.sum())} of {bad.numel()} pixels differ, first at {bad.nonzero()[:4].tolist()}"


def _entry(frames, frame_no, marks, timeline, strip):
    """gcv_scan_annotate through the C ABI, for rows the binding refuses: frames on the device -> a new tensor"""
    nf, h, w, _ = frames.shape
    fd = torch.tensor(frame_no, dtype=torch.int32, device="cuda")
    md = torch.tensor(marks, dtype=torch.int32, device="cuda").reshape(-1, 8)
    tl = (timeline & 0xFFFFFF).to(torch.int32).cuda()
    out = torch.empty_like(frames)
    _lib.check(_lib.load().gcv_scan_annotate(frames.data_ptr(), nf, h, w, fd.data_ptr(), md.data_ptr(), md.shape[0],
                                             tl.data_ptr(), tl.shape[0], tl.shape[1], strip, out.data_ptr(),
                                             _lib.current_stream_ptr(frames.device)), "gcv_scan_annotate")
    return out


def _check(frames, frame_no, marks, timeline, strip, entry=False):
    tl = None if timeline is None else timeline.cuda()
    got = (_entry(frames.cuda(), frame_no, marks, timeline, strip) if entry
           else _lib.scan_annotate(frames.cuda(), frame_no, marks, tl, strip)).cpu()
    _same(got, au.annotate_ref(frames, frame_no, marks, timeline, strip))
    return got


# ----------------------------------------------------------------------------- the kernel
@pytest.mark.parametrize("name", NAMES)
def test_scan_annotate_is_bit_equal_to_the_restatement(name):
    """Tiny frames, several in one block; rows and frames that end inside a piece; 300 marks (more than one ballot round,
    most blocks untouched); overlapping and nested marks in row order; 1 x 1 boxes and outlines that fill their box; every
    label length, clipped tabs, both inks and the luma-128 boundary; T in {1, 5, W, 4 W + 3}, 1 ... 8 lanes, strips from
    one row a lane to the whole frame, frame_no of -1, T - 1 and T; one full-HD group with the default strip.  The rows
    that draw nothing — the binding refuses them — go through the C entry, among rows that draw."""
    frames, frame_no, marks, timeline, strip = _case(name)
    got = _check(frames, frame_no, marks, timeline, strip, entry=name == au.RAW)
    if marks or strip:
        assert not torch.equal(got, frames)


def test_scan_annotate_alignment_and_buffers():
    frames, frame_no, marks, timeline, strip = _case("tiny frames")
    want = au.annotate_ref(frames, frame_no, marks, timeline, strip)
    tl = timeline.cuda()
    # a slab one byte into its allocation, read and written there
    raw = torch.zeros(frames.numel() + 1, dtype=torch.uint8, device="cuda")
    odd = raw[1:].view(frames.shape)
    odd.copy_(frames)
    assert odd.data_ptr() % 4 == 1
    _same(_lib.scan_annotate(odd, frame_no, marks, tl, strip).cpu(), want)
    assert torch.equal(odd.cpu(), frames) and int(raw[0]) == 0
    assert _lib.scan_annotate(odd, frame_no, marks, tl, strip, out=odd) is odd
    _same(odd.cpu(), want)
    assert int(raw[0]) == 0
    # out given; in place; n = 0 and strip = 0 into another buffer is a copy, in place it is nothing
    fd = frames.cuda()
    out = torch.full(frames.shape, 7, dtype=torch.uint8, device="cuda")
    assert _lib.scan_annotate(fd, frame_no, marks, tl, strip, out=out) is out
    _same(out.cpu(), want)
    assert torch.equal(fd.cpu(), frames)
    assert _lib.scan_annotate(fd, frame_no, [], None, 0, out=out) is out and torch.equal(out.cpu(), frames)
    assert _lib.scan_annotate(fd, frame_no, [], None, 0, out=fd) is fd and torch.equal(fd.cpu(), frames)
    assert torch.equal(_lib.scan_annotate(fd, frame_no, []).cpu(), frames)
    assert _lib.scan_annotate(fd, frame_no, marks, tl, strip, out=fd) is fd
    _same(fd.cpu(), want)
    with pytest.raises(_lib.GenConViTHipError):
        _lib.scan_annotate(fd, frame_no, marks, tl, strip, out=torch.empty((5, 37, 54, 3), dtype=torch.uint8, device="cuda"))
    # in place with most blocks untouched: the others keep their bytes
    frames, frame_no, marks, timeline, strip = _case("many marks")
    fd = frames.cuda()
    _lib.scan_annotate(fd, frame_no, marks, None, 0, out=fd)
    _same(fd.cpu(), au.annotate_ref(frames, frame_no, marks, None, 0))


def test_scan_annotate_non_contiguous_frames():
    big = au.frames_of((2, 70, 110, 3), 300)
    view = big[:, 5:66, 10:101]
    marks = au.random_marks(2, 61, 91, 12, 301)
    tl = au.timeline_of(3, 7, 302)
    got = _lib.scan_annotate(big.cuda()[:, 5:66, 10:101], [6, 2], marks, tl.cuda(), 6)
    _same(got.cpu(), au.annotate_ref(view, [6, 2], marks, tl, 6))


# ----------------------------------------------------------------------------- render_scan end to end
_MODELS = {}
MAX_BATCH = 8


def _model(kind):
    if kind not in _MODELS:
        dtype = torch.float32 if kind == "ed fp32" else torch.float16
        ed = GenConViTED(load_config(), init="empty")
        ed.load_state_dict(synthetic_sd("ed"))
        ed = ed.to("cuda").to(dtype).eval()
        if kind == "ed fp32":
            _MODELS[kind] = GenConViT.from_modules(ed, None, net="ed")
        else:
            vae = GenConViTVAE(load_config(), init="empty")
            vae.load_state_dict(synthetic_sd("vae"), strict=False)
            vae.keep_kl_weights = False
            _MODELS[kind] = GenConViT.from_modules(ed, vae.to("cuda").to(dtype).eval(), net="genconvit")
    return _MODELS[kind]


def _scene():
    """24 frames of 96 x 128; track 0 on frames 0 ... 9, track 1 beside it on frames 4 ... 20; frames 21 ... 23 faceless"""
    frames = au.frames_of((24, 96, 128, 3), 310)
    boxes = [(f, 30, 126, 80, 76 + f) for f in range(10)]
    boxes += [(f, 6 + f % 3, 70 + f % 2, 70 + f % 3, 8 + f % 2) for f in range(4, 21)]
    return frames, boxes


def _compose(frames, res, model, eps, ids_of_group, layer, which):
    """What render_scan has to return: per group of evidence rows one ``model.explain`` and one ``_lib.cam_overlay`` on the
    device, then the restatement over marks and a timeline built here from ``res``."""
    rows, off = res["boxes"], res["track_offsets"]
    track_of = [t for t in range(len(off) - 1) for _ in range(off[t + 1] - off[t])]
    dev = frames.cuda()
    p = next(model.parameters())
    for ids in [g[s:s + MAX_BATCH] for g in ids_of_group for s in range(0, len(g), MAX_BATCH)]:
        full = ids + ids[-1:] * (MAX_BATCH - len(ids))                      # render_scan fills every call up to max_batch
        x = _lib.face_crop_preprocess(dev, [rows[i] for i in full], dtype=p.dtype)
        _, cams = model.explain(x, eps=None if eps is None else eps[full], upsample=False, layer=layer)
        _lib.cam_overlay(dev, [rows[i] for i in ids], pred_func._overlay_maps(model, cams, which)[:len(ids)], 0.5, True, None,
                         out=dev)
    lut = _lib.jet_lut()
    k = torch.round(res["frame_scores"][:, 0].float().cpu() * 255.0).long().tolist()
    colour = lambda kk: au.pack(*lut[kk].tolist())
    marks = [(*b, colour(k[i]), 1, track_of[i]) for i, b in enumerate(rows)]
    nf = len(frames)
    tl = torch.tensor([[0x404040] * nf, [0x202020] * nf], dtype=torch.int64)
    for f in range(nf):
        here = [k[i] for i, b in enumerate(rows) if b[0] == f]
        if here:
            tl[0, f] = colour(max(here))
        if any(a <= f <= z for _, a, z, _ in res["segments"]):
            tl[1, f] = 0x0000FF
    return au.annotate_ref(dev.cpu(), list(range(nf)), marks, tl, 4)


@pytest.mark.parametrize("kind", ["ed fp32", "genconvit fp16"])
def test_render_scan_on_the_device(kind):
    """The scan's own ``res``, with a FAKE segment on frames 8 ... 14 of track 1 added where the synthetic weights give
    none there, so that evidence is drawn whatever they say."""
    model = _model(kind)
    frames, boxes = _scene()
    eps = None if kind == "ed fp32" else synth.make_eps(27, name="render").cuda()
    res = pred_func.scan_frames(frames.numpy(), model, boxes=boxes, window=5, stride=2, eps=eps)
    assert res["track_offsets"] == [0, 10, 27] and res["boxes"] == boxes
    print(f"\n{kind}: segments of the scan {res['segments']}")
    res = dict(res, segments=list(res["segments"]) + [(1, 8, 14, 1.0)])
    rows = res["boxes"]
    ev = sorted({i for t, a, z, _ in res["segments"] for i in range(res["track_offsets"][t], res["track_offsets"][t + 1])
                 if a <= rows[i][0] <= z})
    assert set(range(14, 21)) <= set(ev)
    layer, which = ("s3", "mean") if kind == "ed fp32" else ("s2", "vae")
    got = pred_func.render_scan(frames.numpy(), res, model, eps=eps, layer=layer, which=which, max_batch=MAX_BATCH)
    assert got.dtype == torch.uint8 and not got.is_cuda
    _same(got, _compose(frames, res, model, eps, [ev], layer, which))
    plain = pred_func.render_scan(frames.cuda(), res, None)
    differs = (got != plain).any(-1).flatten(1).any(1).tolist()
    assert differs == [f in {rows[i][0] for i in ev} for f in range(24)]
    # groups of 5 frames: each group's evidence rows are one explain call of their own, filled up to max_batch rows, so
    # the 16-bit networks run the kernels of one batch size and the frames are the same
    seen = []
    assert pred_func.render_scan(frames.cuda(), res, model, eps=eps, layer=layer, which=which, max_frames=5, max_batch=MAX_BATCH,
                                 sink=lambda g, slab: seen.append((g, slab))) is None
    assert [g for g, _ in seen] == [0, 5, 10, 15, 20] and all(s.is_cuda for _, s in seen)
    grouped = torch.cat([s for _, s in seen]).cpu()
    by_group = [[i for i in ev if g <= rows[i][0] < g + 5] for g in range(0, 24, 5)]
    _same(grouped, _compose(frames, res, model, eps, [ids for ids in by_group if ids], layer, which))
    _same(grouped, got)
