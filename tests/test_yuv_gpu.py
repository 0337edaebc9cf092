"""gcv_yuv420_to_rgb and gcv_rgb_to_yuv420 on the MI355X against their CPU restatement (tests/yuvutil.py): torch.equal on
every byte of every case under both layouts, both matrices and both ranges — no tolerance, no excluded pixels —, the
alignments a packed stream and a view can have, ``out=``, the rows the C entries refuse; then ``pred_func.scan_frames`` and
``render_scan`` end to end with synthetic weights: decoder-native frames in a ``YUV420`` against the same pixels given as
host RGB frames, exactly.  Which defects these comparisons catch: tests/test_yuv_sensitivity_cpu.py."""
import functools
import itertools

import numpy as np
import pytest
import torch

from genconvit_amd import _lib, synth
from genconvit_amd.model import pred_func
from genconvit_amd.model.config import load_config
from genconvit_amd.model.genconvit import GenConViT
from genconvit_amd.model.genconvit_ed import GenConViTED
from genconvit_amd.model.genconvit_vae import GenConViTVAE
from tests import yuvutil as yu
from tests.conftest import synthetic_sd

pytestmark = pytest.mark.gpu
torch.set_grad_enabled(False)

COLOURS = list(itertools.product(yu.MATRICES, yu.RANGES))


def _same(got, want, what):
    got, want = got.cpu(), torch.as_tensor(want)
    bad = got != want
    assert got.shape == want.shape and torch.equal(got, want), \
        f"{what}: {int(bad.sum())} of {bad.numel()} bytes differ, first at {bad.nonzero()[:4].tolist()}"


# ----------------------------------------------------------------------------- the kernels
@pytest.mark.parametrize("layout", yu.LAYOUTS)
@pytest.mark.parametrize("name", yu.CASES_IN)
def test_yuv420_to_rgb_is_bit_equal_to_the_restatement(name, layout):
    """Random bytes (both clips of every channel) at F = 3 and 2 x 2 ... 10 x 34: frames that start at 0 and 2 mod 4 and widths
    2, 6, 0 mod 8; the 256 x 25 table; flat frames at the range corners; 2 frames of 720p on the aligned path."""
    yuv = yu.case_in(name, layout)
    dev = torch.as_tensor(yuv).cuda()
    for matrix, full in COLOURS:
        _same(_lib.yuv420_to_rgb(dev, layout, matrix, full), yu.to_rgb_ref(yuv, layout, matrix, full), (name, layout, matrix, full))


@pytest.mark.parametrize("layout", yu.LAYOUTS)
@pytest.mark.parametrize("name", yu.CASES_OUT)
def test_rgb_to_yuv420_is_bit_equal_to_the_restatement(name, layout):
    """The same sizes; flat colours at the corners of the cube (the chroma clip under full range); blocks of four different
    pixels on both sides of a chroma rounding step; 720p."""
    rgb = yu.case_out(name)
    dev = torch.as_tensor(rgb).cuda()
    for matrix, full in COLOURS:
        _same(_lib.rgb_to_yuv420(dev, layout, matrix, full), yu.to_yuv_ref(rgb, layout, matrix, full), (name, layout, matrix, full))


@pytest.mark.parametrize("layout", yu.LAYOUTS)
def test_every_alignment_of_both_buffers(layout):
    """Views 0 ... 8 bytes into a larger buffer, for the input and for ``out``: every start mod 8, so W % 8 == 0 frames take
    the byte path when either pointer is off; the bytes around ``out`` stay untouched."""
    for h, w in ((4, 16), (6, 10)):
        yuv = yu.case_in(f"rand_{h}x{w}", layout)
        rgb = yu.case_out(f"rand_{h}x{w}")
        want_rgb, want_yuv = yu.to_rgb_ref(yuv, layout, "bt601", True), yu.to_yuv_ref(rgb, layout, "bt601", True)
        for a, b in itertools.product(range(9), (0, 1, 4, 8)):
            for src, want, call in ((yuv, want_rgb, _lib.yuv420_to_rgb), (rgb, want_yuv, _lib.rgb_to_yuv420)):
                big = torch.full((src.size + 16,), 7, dtype=torch.uint8, device="cuda")
                big[a:a + src.size] = torch.as_tensor(src).cuda().reshape(-1)
                land = torch.full((want.size + 16,), 9, dtype=torch.uint8, device="cuda")
                out = land[b:b + want.size].view(want.shape)
                assert call(big[a:a + src.size].view(src.shape), layout, "bt601", True, out=out) is out
                _same(out, want, (call.__name__, h, w, a, b))
                assert bool((land[:b] == 9).all()) and bool((land[b + want.size:] == 9).all())


def test_out_views_and_no_frames():
    yuv, rgb = yu.case_in("rand_6x10", "nv12"), yu.case_out("rand_6x10")
    dy, dr = torch.as_tensor(yuv).cuda(), torch.as_tensor(rgb).cuda()
    slab = torch.zeros((5, 6, 10, 3), dtype=torch.uint8, device="cuda")
    assert _lib.yuv420_to_rgb(dy[1:], "nv12", out=slab[2:4]).data_ptr() == slab[2:4].data_ptr()
    _same(slab[2:4], yu.to_rgb_ref(yuv[1:], "nv12"), "rows of a larger slab")
    assert not bool(slab[:2].any()) and not bool(slab[4:].any())
    planes = torch.zeros((5, 9, 10), dtype=torch.uint8, device="cuda")
    _lib.rgb_to_yuv420(dr[:2], "i420", out=planes[3:])
    _same(planes[3:], yu.to_yuv_ref(rgb[:2], "i420"), "rows of a larger buffer")
    assert not bool(planes[:3].any())
    assert tuple(_lib.yuv420_to_rgb(dy[:0]).shape) == (0, 6, 10, 3) and tuple(_lib.rgb_to_yuv420(dr[:0]).shape) == (0, 9, 10)
    for bad in (slab[:3].float(), slab[:2], slab[:3, :, :, :2], slab[:3].cpu(), slab[:3].permute(0, 2, 1, 3)):
        with pytest.raises(_lib.GenConViTHipError, match="yuv420_to_rgb: out"):
            _lib.yuv420_to_rgb(dy, "nv12", out=bad)
    with pytest.raises(_lib.GenConViTHipError, match="rgb_to_yuv420: out"):
        _lib.rgb_to_yuv420(dr, out=planes[:3, :8])
    for call, bad in ((_lib.yuv420_to_rgb, dy.cpu()), (_lib.rgb_to_yuv420, dr.cpu())):
        with pytest.raises(_lib.GenConViTHipError, match="no CPU path"):
            call(bad)


def test_the_c_entries_and_what_they_refuse():
    """Once each through the raw C ABI; the refused rows never reach a launch and say why."""
    lib, stream = _lib.load(), _lib.current_stream_ptr(torch.device("cuda"))
    yuv, rgb = yu.case_in("rand_6x10", "nv12"), yu.case_out("rand_6x10")
    dy, dr = torch.as_tensor(yuv).cuda(), torch.as_tensor(rgb).cuda()
    out_rgb, out_yuv = torch.full_like(dr, 3), torch.full_like(dy, 3)
    to_rgb = lambda nf=3, h=6, w=10, lay=1, mat=1, full=0, src=dy.data_ptr(), dst=out_rgb.data_ptr(): \
        lib.gcv_yuv420_to_rgb(src, nf, h, w, lay, mat, full, dst, stream)
    to_yuv = lambda nf=3, h=6, w=10, lay=1, mat=1, full=0, src=dr.data_ptr(), dst=out_yuv.data_ptr(): \
        lib.gcv_rgb_to_yuv420(src, nf, h, w, lay, mat, full, dst, stream)
    for call, name in ((to_rgb, "gcv_yuv420_to_rgb"), (to_yuv, "gcv_rgb_to_yuv420")):
        for kw in (dict(h=5), dict(w=9), dict(h=0), dict(w=0), dict(h=-6), dict(w=-10), dict(lay=2), dict(lay=-1), dict(mat=2),
                   dict(mat=-1), dict(nf=-1), dict(src=None), dict(dst=None), dict(h=65538), dict(nf=1 << 20, h=64, w=64)):
            assert call(**kw) != 0, (name, kw)
            with pytest.raises(_lib.GenConViTHipError, match="yuv420"):
                _lib.check(call(**kw), name)
        assert call(nf=0) == 0 and call(nf=0, src=None, dst=None) == 0
    torch.cuda.synchronize()
    assert bool((out_rgb == 3).all()) and bool((out_yuv == 3).all())           # nothing was launched so far
    _lib.check(to_rgb(), "gcv_yuv420_to_rgb")
    _lib.check(to_yuv(full=7), "gcv_rgb_to_yuv420")                            # any non-zero full_range is full range
    _same(out_rgb, yu.to_rgb_ref(yuv, "nv12", "bt709", False), "C entry, to rgb")
    _same(out_yuv, yu.to_yuv_ref(rgb, "nv12", "bt709", True), "C entry, to yuv")


# ----------------------------------------------------------------------------- scan_frames and render_scan end to end
@functools.lru_cache(maxsize=None)
def _model():
    dtype = torch.float16
    ed = GenConViTED(load_config(), init="empty")
    ed.load_state_dict(synthetic_sd("ed"))
    vae = GenConViTVAE(load_config(), init="empty")
    vae.load_state_dict(synthetic_sd("vae"), strict=False)
    vae.keep_kl_weights = False
    return GenConViT.from_modules(ed.to("cuda").to(dtype).eval(), vae.to("cuda").to(dtype).eval(), net="genconvit")


@functools.lru_cache(maxsize=None)
def _scene():
    """16 frames of 96 x 128 as nv12 bt601 full-range bytes: a smooth drifting background and a 64 x 64 patch of 4-pixel
    texture that moves 4 pixels — one cell of a 16 x 16 grid — a frame; boxes on every 4th frame (detect_every = 4: the
    frames between are filled and followed, the three after a shot's last box reached by extension); a hard cut to
    another background and patch at frame 8."""
    rng = np.random.default_rng(5)
    yy, xx = np.mgrid[0:96, 0:128]
    patches = [rng.integers(0, 256, size=(16, 16, 3)).repeat(4, 0).repeat(4, 1) for _ in range(2)]
    left = lambda f: 4 + 20 * (f // 8) + 4 * (f % 8)
    frames = np.empty((16, 96, 128, 3), dtype=np.uint8)
    for f in range(16):
        shot = f // 8
        back = np.stack([(90 + 60 * shot + xx // 2 + f) % 256, (40 + 100 * shot + yy + 2 * f) % 256, (200 - 90 * shot + (xx + yy) // 4) % 256], -1)
        back[16:80, left(f):left(f) + 64] = patches[shot]
        frames[f] = (back + rng.integers(-3, 4, size=back.shape)).clip(0, 255)
    boxes = [(f, 16, left(f) + 64, 80, left(f)) for f in (0, 4, 8, 12)]
    return yu.to_yuv_ref(frames, "nv12", "bt601", True), boxes


COLOUR = dict(layout="nv12", matrix="bt601", full_range=True)
SCAN = dict(detect_every=4, window=4, stride=2, max_batch=5, follow=True, follow_grid=16, follow_radius=4, cuts=True,
            transitions=True, quality=True, quality_args=dict(grid=16), persons=True, extend=True,
            extend_args=dict(grid=16, radius=4, steps=3))


def _assert_equal(a, b, path="res"):
    assert type(a) is type(b) or (isinstance(a, (int, float)) and isinstance(b, (int, float))), (path, type(a), type(b))
    if torch.is_tensor(a):
        assert a.device == b.device and a.dtype == b.dtype and torch.equal(a, b), path
    elif isinstance(a, np.ndarray):
        assert a.dtype == b.dtype and np.array_equal(a, b, equal_nan=a.dtype.kind == "f"), path
    elif isinstance(a, dict):
        assert a.keys() == b.keys(), (path, sorted(a), sorted(b))
        for k in a:
            _assert_equal(a[k], b[k], f"{path}[{k!r}]")
    elif isinstance(a, (list, tuple)):
        assert len(a) == len(b), path
        for i, (x, y) in enumerate(zip(a, b)):
            _assert_equal(x, y, f"{path}[{i}]")
    else:
        assert a == b, (path, a, b)


@functools.lru_cache(maxsize=None)
def _scans():
    """(the scan of the RGB restatement of the scene given as host frames, the eps it ran with)"""
    yuv, boxes = _scene()
    rgb = yu.to_rgb_ref(yuv, **COLOUR)
    model = _model()
    probe = pred_func.scan_frames(rgb, model, boxes=boxes, **dict(SCAN, persons=None))
    eps = synth.make_eps(len(probe["boxes"]), name="yuv scan").cuda()
    return pred_func.scan_frames(rgb, model, boxes=boxes, eps=eps, **SCAN), eps


@pytest.mark.parametrize("where", ["host numpy", "host tensor", "device"])
def test_scan_frames_from_yuv_equals_the_scan_of_the_same_pixels(where):
    """Equal slabs and equal groups make this exact: every stage that is on sees, per group, the slab host RGB frames
    would have given it."""
    yuv, boxes = _scene()
    want, eps = _scans()
    print(f"\n{len(want['tracks'])} tracks, {len(want['boxes'])} crops, {want['follow'].shape[0]} follow jobs, "
          f"{want['extend'].shape[0]} extension steps, cuts {want['cuts']}, transitions {want['transitions']}")
    assert want["follow"].shape[0] >= 3 and want["extend"].shape[0] >= 1 and want["cuts"] == [8]        # every stage had work
    assert len(want["boxes"]) == eps.shape[0] >= 8 and {"persons", "quality", "transitions", "cut_scores"} <= set(want)
    data = {"host numpy": yuv, "host tensor": torch.as_tensor(yuv), "device": torch.as_tensor(yuv).cuda()}[where]
    got = pred_func.scan_frames(pred_func.YUV420(data, **COLOUR), _model(), boxes=boxes, eps=eps, **SCAN)
    _assert_equal(got, want)


def test_scan_frames_hands_the_detector_rgb_frames():
    yuv, boxes = _scene()
    rgb = yu.to_rgb_ref(yuv, **COLOUR)
    seen = []

    def locate(frames):
        seen.append(np.array(frames))
        return [(k, *boxes[k][1:]) for k in range(len(frames))]
    kw = dict(locate=locate, detect_every=4, window=4, stride=2, max_batch=3)
    got = pred_func.scan_frames(pred_func.YUV420(yuv, **COLOUR), _model(), **kw)
    want = pred_func.scan_frames(rgb, _model(), **kw)
    assert seen[0].dtype == np.uint8 and np.array_equal(seen[0], rgb[::4]) and np.array_equal(seen[1], rgb[::4])
    assert got["boxes"] == want["boxes"] and len(got["boxes"]) >= 4


@pytest.mark.parametrize("where", ["host", "device"])
def test_render_scan_from_yuv_to_nv12(where):
    yuv, boxes = _scene()
    res, eps = _scans()
    res = dict(res, segments=list(res["segments"]) + [(0, 2, 6, 1.0)])          # evidence is drawn whatever the weights say
    model = _model()
    rgb = yu.to_rgb_ref(yuv, **COLOUR)
    kw = dict(eps=eps, max_frames=6, max_batch=4, layer="s2", which="vae")
    drawn = pred_func.render_scan(rgb, res, model, **kw)
    assert not torch.equal(drawn, torch.as_tensor(rgb))
    fr = pred_func.YUV420(yuv if where == "host" else torch.as_tensor(yuv).cuda(), **COLOUR)
    got = pred_func.render_scan(fr, res, model, out="nv12", **kw)
    assert got.dtype == torch.uint8 and not got.is_cuda
    _same(got, yu.to_yuv_ref(drawn.numpy(), **COLOUR), "render_scan out=nv12")
    _same(pred_func.render_scan(fr, res, model, **kw), drawn, "render_scan from YUV, out=rgb")
    groups = []
    assert pred_func.render_scan(rgb, res, model, out="i420", out_matrix="bt709", sink=lambda g, s: groups.append((g, s)), **kw) is None
    assert [g for g, _ in groups] == [0, 6, 12] and all(s.is_cuda for _, s in groups)
    _same(torch.cat([s for _, s in groups]), yu.to_yuv_ref(drawn.numpy(), "i420", "bt709", False), "render_scan sink, i420")


def test_explain_frames_takes_yuv():
    yuv, boxes = _scene()
    rgb = yu.to_rgb_ref(yuv, **COLOUR)
    model, eps = _model(), synth.make_eps(4, name="yuv explain").cuda()
    v0, o0, b0 = pred_func.explain_frames(rgb, model, boxes=boxes, eps=eps)
    v1, o1, b1 = pred_func.explain_frames(pred_func.YUV420(yuv, **COLOUR), model, boxes=boxes, eps=eps)
    assert v0 == v1 and b0 == b1 and torch.equal(o0, o1)
