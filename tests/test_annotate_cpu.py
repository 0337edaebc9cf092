"""The scan's drawing without a GPU: the CPU restatement of gcv_scan_annotate's arithmetic (tests/annotateutil.py) against
expectations written out by hand, the argument checks of ``_lib.scan_annotate``, which all run before the library is
loaded, and ``pred_func.render_scan`` / ``render_video`` end to end with the three device entries replaced by their
restatements and a stand-in model whose maps are a known function of the crop."""
import os
import re

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from genconvit_amd import _lib
from genconvit_amd.model import pred_func
from genconvit_amd.model.genconvit import normalize_cams
from tests import annotateutil as au
from tests import overlayutil as ou
from tests import scanutil as su

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
torch.set_grad_enabled(False)


def test_header_declares_gcv_scan_annotate_and_the_binding_knows_it():
    hdr = open(os.path.join(REPO, "include", "genconvit_hip.h")).read()
    assert re.search(r"\bint\s+gcv_scan_annotate\s*\(", hdr)
    assert len(_lib.SIGNATURES["gcv_scan_annotate"][1]) == 13


# ----------------------------------------------------------------------------- annotate_ref by hand
LABEL_40 = [                       # a 16 x 30 box, thick 2, label 40: # the mark's colour, k ink, . the frame
    "##############################",
    "##############################",
    "##kk##kk##kkkkkk##..........##",
    "##kk##kk##kkkkkk##..........##",
    "##kk##kk##kk##kk##..........##",
    "##kk##kk##kk##kk##..........##",
    "##kkkkkk##kk##kk##..........##",
    "##kkkkkk##kk##kk##..........##",
    "######kk##kk##kk##..........##",
    "######kk##kk##kk##..........##",
    "######kk##kkkkkk##..........##",
    "######kk##kkkkkk##..........##",
    "##################..........##",
    "##################..........##",
    "##############################",
    "##############################",
]


def _picture(out, frames, f, top, right, bottom, left, colour):
    """The box of ``out`` as rows of '#', 'k' (black), 'w' (white), '.' (the frame's own pixel), '?' anything else."""
    col, rows = list(au.rgb(colour)), []
    for y in range(top, bottom):
        row = ""
        for x in range(left, right):
            p = out[f, y, x].tolist()
            row += "#" if p == col else "k" if p == [0, 0, 0] else "w" if p == [255] * 3 else "." \
                if p == frames[f, y, x].tolist() else "?"
        rows.append(row)
    return rows


def _mid_frames(shape, seed):
    """Random pixels in 1 ... 254 with red != green: no pixel is black, white or grey, so a picture's letters are unambiguous"""
    fr = torch.randint(1, 255, shape, dtype=torch.uint8, generator=torch.Generator().manual_seed(seed))
    fr[..., 1] = torch.where(fr[..., 1] == fr[..., 0], fr[..., 1] ^ 1, fr[..., 1]).clamp(1, 254)
    return fr


def test_label_40_is_this_bitmap():
    frames = _mid_frames((2, 24, 40, 3), 1)
    out = au.annotate_ref(frames, [0, 1], [(1, 3, 36, 19, 6, 0x00FF00, 2, 40)])
    assert _picture(out, frames, 1, 3, 36, 19, 6, 0x00FF00) == LABEL_40
    keep = torch.ones((2, 24, 40), dtype=torch.bool)
    keep[1, 3:19, 6:36] = False
    assert torch.equal(out[keep], frames[keep])                              # nothing outside the box


def test_every_digit_reads_as_the_font_says():
    frames = _mid_frames((1, 9, 45, 3), 2)
    for label in (0, 19, 283, 745, 6):
        nd = len(str(label))
        out = au.annotate_ref(frames, [0], [(0, 1, 44, 8, 1, 0x0000FF, 1, label)])
        got = _picture(out, frames, 0, 1, 4 * nd + 2, 8, 1, 0x0000FF)      # red: luma 76, white ink
        for k, d in enumerate(str(label)):
            assert ["".join("1" if c == "w" else "0" for c in row[1 + 4 * k:4 + 4 * k]) for row in got[1:6]] == \
                   [au.FONT[int(d)][3 * r:3 * r + 3] for r in range(5)], (label, k)
        assert all(row[4 * k] == "#" for row in got for k in range(nd + 1)) and set(got[0] + got[6]) == {"#"}


def test_a_one_pixel_box_and_a_box_its_outline_fills():
    frames = _mid_frames((1, 30, 30, 3), 3)
    out = au.annotate_ref(frames, [0], [(0, 4, 6, 5, 5, 0x112233, 1, -1), (0, 8, 28, 28, 8, 0x445566, 16, -1),
                                        (0, 2, 20, 6, 10, 0x778899, 2, -1), (0, 20, 5, 29, 0, 0xAABBCC, 3, 0)])
    assert out[0, 4, 5].tolist() == [0x33, 0x22, 0x11]
    assert _picture(out, frames, 0, 8, 28, 28, 8, 0x445566) == ["#" * 20] * 20            # thick 16 on 20 x 20
    assert _picture(out, frames, 0, 2, 20, 6, 10, 0x778899) == ["#" * 10] * 4              # 2 thick == the height
    # 9 x 5 at thick 3, label 0: 2 thick >= the width, and the tab (21 x 15) is clipped by the box
    assert _picture(out, frames, 0, 20, 5, 29, 0, 0xAABBCC) == ["#####"] * 3 + ["###kk"] * 6
    changed = (out != frames).any(-1)
    assert int(changed.sum()) == 1 + 400 + 40 + 45


@pytest.mark.parametrize("grey, ink", [(128, "k"), (127, "w")])
def test_ink_colour_at_the_luma_boundary(grey, ink):
    assert (77 * grey + 150 * grey + 29 * grey) >> 8 == grey
    frames = _mid_frames((1, 9, 9, 3), 4)
    colour = au.pack(grey, grey, grey)
    got = _picture(au.annotate_ref(frames, [0], [(0, 0, 9, 9, 0, colour, 1, 1)]), frames, 0, 0, 9, 9, 0, colour)
    assert got[1:6] == [f"##{ink}##...#", f"#{ink}{ink}##...#", f"##{ink}##...#", f"##{ink}##...#", f"#{ink}{ink}{ink}#...#"]


@pytest.mark.parametrize("T", [1, 5, 53, 4 * 53 + 3])
def test_cursor_widths(T):
    W, H, strip = 53, 12, 4
    tl = torch.full((1, T), au.pack(10, 20, 30), dtype=torch.int64)
    cs = sorted({0, T // 2, T - 1})
    frames = _mid_frames((len(cs) + 2, H, W, 3), 5)
    out = au.annotate_ref(frames, cs + [-1, T], [], tl, strip)
    assert torch.equal(out[:, :H - strip], frames[:, :H - strip])
    for f, c in enumerate(cs):
        white = (out[f, H - strip:] == 255).all(-1)
        assert (white == white[0]).all()
        cols = white[0].nonzero().flatten().tolist()
        x0 = c * W // T
        want = list(range(x0, max(x0 + 1, (c + 1) * W // T)))
        assert cols == want and len(cols) >= 1, (T, c, cols)
        assert len(cols) in {1: (53,), 5: (10, 11), 53: (1,), 4 * 53 + 3: (1,)}[T]
        assert (out[f, H - strip:][~white] == torch.tensor([10, 20, 30], dtype=torch.uint8)).all()
    for f in (len(cs), len(cs) + 1):                                         # frame_no -1 and T: no cursor
        assert (out[f, H - strip:] == torch.tensor([10, 20, 30], dtype=torch.uint8)).all()


def test_timeline_lanes_columns_and_order_over_the_marks():
    H, W, strip = 20, 10, 7
    tl = torch.tensor([[au.pack(1, 0, 0), au.pack(2, 0, 0)], [au.pack(3, 0, 0), au.pack(4, 0, 0)],
                       [au.pack(5, 0, 0), au.pack(6, 0, 0) | 0x7F000000]], dtype=torch.int64)
    frames = _mid_frames((1, H, W, 3), 6)
    out = au.annotate_ref(frames, [9], [(0, 0, W, H, 0, 0xFFFFFF, 16, -1)], tl, strip)
    assert (out[0, :H - strip] == 255).all()                                # the mark fills the frame; the strip is over it
    assert out[0, H - strip:, :, 0].tolist() == [[1] * 5 + [2] * 5] * 3 + [[3] * 5 + [4] * 5] * 2 + [[5] * 5 + [6] * 5] * 2
    assert (out[0, H - strip:, :, 1:] == 0).all()                           # lanes (y' 3) // 7 for y' = 0 ... 6: 0 0 0 1 1 2 2


def test_rows_that_draw_nothing_and_row_order():
    frames = _mid_frames((2, 12, 12, 3), 7)
    junk = [(2, 0, 5, 5, 0, 1, 1, 1), (-1, 0, 5, 5, 0, 1, 1, 1), (0, 0, 13, 5, 0, 1, 1, 1), (0, -1, 5, 5, 0, 1, 1, 1),
            (0, 5, 5, 5, 0, 1, 1, 1), (0, 0, 5, 5, 0, 1, 0, 1), (0, 0, 5, 5, 0, 1, 17, 1), (0, 0, 5, 5, 0, 1, 1, 1000),
            (0, 0, 5, 5, 0, 1, 1, -2)]
    assert torch.equal(au.annotate_ref(frames, [0, 1], junk), frames)
    a, b = (0, 1, 9, 9, 1, 0x0000FF, 2, -1), (0, 3, 11, 11, 3, 0x00FF00, 2, -1)
    ab, ba = au.annotate_ref(frames, [0, 1], [a, b]), au.annotate_ref(frames, [0, 1], [b, a])
    assert ab[0, 3, 7].tolist() == [0, 255, 0] and ba[0, 3, 7].tolist() == [255, 0, 0]   # a's right edge, b's top edge
    assert torch.equal(ab, au.annotate_ref(au.annotate_ref(frames, [0, 1], [a]), [0, 1], [b]))


def test_the_shared_cases_are_what_the_gpu_test_says():
    cases = au.cases()
    fr, no, marks, tl, strip = cases["many marks"]
    assert len(marks) == 300 and tuple(fr.shape) == (2, 130, 250, 3)
    touched = (au.annotate_ref(fr, no, marks, tl, strip) != fr).any(-1).flatten()
    blocks = [bool(touched[i:i + 4096].any()) for i in range(0, touched.numel(), 4096)]
    assert len(blocks) == 16 and any(blocks)
    fr, no, marks, tl, strip = cases["tiny frames"]
    assert {m[0] for m in marks if m[0] < 5} == {0, 1, 2, 4} and 5 * 37 * 53 < 3 * 4096
    assert {m[7] for m in cases["labels"][2]} >= {-1, 0, 9, 10, 99, 100, 999}
    assert {au.GREY128, au.GREY127} <= {m[5] for m in cases["labels"][2]}
    assert all(f"width {w}" in cases for w in (1, 2, 3, 5, 641, 1024))
    for name, (fr, no, marks, tl, strip) in cases.items():
        assert len(no) == fr.shape[0], name


# ----------------------------------------------------------------------------- the binding's refusals
def test_scan_annotate_rejects_bad_input_before_the_library_is_loaded(monkeypatch):
    def no_load():
        raise AssertionError("the library was loaded")
    monkeypatch.setattr(_lib, "load", no_load)
    frames = torch.zeros((2, 32, 40, 3), dtype=torch.uint8)
    ok = (1, 2, 12, 12, 2, 0xFF, 1, 7)
    tl = torch.zeros((2, 5), dtype=torch.int64)
    bad = _lib.GenConViTHipError
    with pytest.raises(bad, match="there is no CPU path"):
        _lib.scan_annotate(frames, [0, 1], [ok], tl, 4)                       # everything right but the device
    with pytest.raises(bad, match="uint8 device tensor"):
        _lib.scan_annotate(frames.float(), [0, 1], [ok])
    with pytest.raises(bad, match="uint8 device tensor"):
        _lib.scan_annotate(frames[..., :2], [0, 1], [ok])
    for row in ((1, 2, 41, 12, 2, 0xFF, 1, 7), (2, 2, 12, 12, 2, 0xFF, 1, 7), (1, 12, 12, 12, 2, 0xFF, 1, 7),
                (1, -1, 12, 12, 2, 0xFF, 1, 7)):
        with pytest.raises(bad, match="mark 1 lies outside its 32x40 frame"):
            _lib.scan_annotate(frames, [0, 1], [ok, row])
    for thick in (0, 17, -1):
        with pytest.raises(bad, match="mark 2 has a thick outside 1 ... 16"):
            _lib.scan_annotate(frames, [0, 1], [ok, ok, ok[:6] + (thick, 7)])
    for label in (-2, 1000):
        with pytest.raises(bad, match="mark 0 has a label outside -1 ... 999"):
            _lib.scan_annotate(frames, [0, 1], [ok[:7] + (label,), ok])
    with pytest.raises(bad, match="mark 1 has a colour outside"):
        _lib.scan_annotate(frames, [0, 1], [ok, ok[:5] + (1 << 24, 1, 7)])
    with pytest.raises(bad, match="frame_no must hold 2 integers"):
        _lib.scan_annotate(frames, [0, 1, 2], [ok])
    with pytest.raises(bad, match="frame_no must hold 2 integers"):
        _lib.scan_annotate(frames, [0.5, 1.0], [ok])
    for timeline in (None, torch.zeros((2, 5)), torch.zeros(5, dtype=torch.int64), torch.zeros((2, 5, 1), dtype=torch.int32),
                     [[0] * 5] * 2, torch.zeros((0, 5), dtype=torch.int64), torch.zeros((2, 5), dtype=torch.bool)):
        with pytest.raises(bad, match=r"timeline must be an \(L, T\) integer tensor"):
            _lib.scan_annotate(frames, [0, 1], [ok], timeline, 4)
    with pytest.raises(bad, match="3 lanes on a strip of 2 rows"):
        _lib.scan_annotate(frames, [0, 1], [ok], torch.zeros((3, 5), dtype=torch.int32), 2)
    with pytest.raises(bad, match="9 lanes"):
        _lib.scan_annotate(frames, [0, 1], [ok], torch.zeros((9, 5), dtype=torch.int32), 20)
    with pytest.raises(bad, match="a strip of 33 rows on frames of 32"):
        _lib.scan_annotate(frames, [0, 1], [ok], tl, 33)
    with pytest.raises(bad, match="must stay below 2\\^31"):
        _lib.scan_annotate(frames, [0, 1], [ok], torch.zeros((1, (1 << 31) // 40 + 1), dtype=torch.int8), 4)
    for strip in (-1, 1.5, True):
        with pytest.raises(bad, match="strip .* must be an integer >= 0"):
            _lib.scan_annotate(frames, [0, 1], [ok], tl, strip)
    for out in (torch.zeros((2, 32, 41, 3), dtype=torch.uint8), torch.zeros((2, 32, 40, 3)), "out",
                torch.zeros((2, 32, 40, 6), dtype=torch.uint8)[..., ::2]):
        with pytest.raises(bad, match="out must be a contiguous uint8 tensor of shape"):
            _lib.scan_annotate(frames, [0, 1], [ok], out=out)


# ----------------------------------------------------------------------------- render_scan end to end
F_, H_, W_ = 24, 48, 64


class StandIn(torch.nn.Module):
    """net "ed"; explain() returns as the original-frame map the 7 x 7 means of the crop's red channel, and records its calls"""
    net = "ed"

    def __init__(self):
        super().__init__()
        self.w = torch.nn.Parameter(torch.zeros(1))
        self.calls = []

    @staticmethod
    def maps(x):
        return F.adaptive_avg_pool2d(x[:, 0].float(), 7)

    def explain(self, x, eps=None, target=None, upsample=True, layer="s3"):
        assert upsample is False and layer == "s2" and x.dtype == torch.float32 and tuple(x.shape[1:]) == (3, 224, 224)
        self.calls.append((x.shape[0], None if eps is None else eps[:, 0].tolist()))
        m = self.maps(x)
        return torch.zeros((x.shape[0], 2)), {"ed": torch.stack((torch.zeros_like(m), m), 1)}


def _scene():
    """Two tracks on 24 frames of 48 x 64: track 0 on frames 4 ... 20 with a FAKE segment on 8 ... 14, track 1 on 0 ... 9,
    overlapping track 0's boxes; frames 21 ... 23 are faceless"""
    frames = au.frames_of((F_, H_, W_, 3), 200)
    t0 = [(f, 4 + f % 3, 40 + f % 2, 36 + f % 3, 8 + f % 2) for f in range(4, 21)]
    t1 = [(f, 20, 62, 44, 30 + f) for f in range(10)]
    g = torch.Generator().manual_seed(201)
    p = torch.rand((len(t0) + len(t1), 1), generator=g)
    res = {"tracks": [t0, t1], "boxes": t0 + t1, "track_offsets": [0, len(t0), len(t0) + len(t1)],
           "frame_scores": torch.cat((p, 1 - p), 1), "segments": [(0, 8, 14, 0.9)], "windows": [], "verdict": (0, 0.7)}
    return frames, res


@pytest.fixture()
def on_the_cpu(monkeypatch):
    """The three device entries behind render_scan, replaced by their restatements"""
    def cam_overlay(frames, boxes, maps, alpha=0.5, weighted=True, lut=None, out=None):
        return out.copy_(ou.overlay_ref(frames, boxes, maps, alpha, weighted, lut))

    def scan_annotate(frames, frame_no, marks, timeline=None, strip=0, out=None):
        return out.copy_(au.annotate_ref(frames, frame_no, marks, timeline, strip))
    monkeypatch.setattr(_lib, "face_crop_preprocess", lambda fr, boxes, size=224, dtype=None: su.face_crop_preprocess_ref(fr, boxes, size, dtype))
    monkeypatch.setattr(_lib, "cam_overlay", cam_overlay)
    monkeypatch.setattr(_lib, "scan_annotate", scan_annotate)


def _compose(frames, res, evidence=True, names=None, thick=1, strip=4, alpha=0.5, lut=None):
    """What render_scan has to return, built from ``res`` here: overlays on the rows inside a segment of their own track,
    then one mark per crop row, then the timeline."""
    rows, off = res["boxes"], res["track_offsets"]
    track_of = [t for t in range(len(off) - 1) for _ in range(off[t + 1] - off[t])]
    table = ou.jet_lut_ref() if lut is None else lut
    k = [int(round(float(np.float32(s) * np.float32(255.0)))) for s in res["frame_scores"][:, 0].tolist()]
    colour = lambda kk: au.pack(*table[kk].tolist())
    out = frames.clone()
    if evidence:
        ev = [i for i, b in enumerate(rows) if any(t == track_of[i] and a <= b[0] <= z for t, a, z, _ in res["segments"])]
        if ev:
            boxes = [rows[i] for i in ev]
            maps = normalize_cams(StandIn.maps(su.face_crop_preprocess_ref(frames, boxes, 224, torch.float32)))
            out = ou.overlay_ref(out, boxes, maps, alpha, True, lut)
    names = list(range(len(off) - 1)) if names is None else names
    marks = [(*b, colour(k[i]), thick, names[track_of[i]]) for i, b in enumerate(rows)]
    tl = torch.tensor([[0x404040] * len(frames), [0x202020] * len(frames)], dtype=torch.int64)
    for f in range(len(frames)):
        here = [k[i] for i, b in enumerate(rows) if b[0] == f]
        if here:
            tl[0, f] = colour(max(here))
        if any(a <= f <= z for _, a, z, _ in res["segments"]):
            tl[1, f] = 0x0000FF
    return au.annotate_ref(out, list(range(len(frames))), marks, tl if strip else None, strip)


def test_render_scan_is_the_composition_of_overlays_marks_and_timeline(on_the_cpu):
    frames, res = _scene()
    model = StandIn()
    keep = frames.clone()
    got = pred_func.render_scan(frames.numpy(), res, model, layer="s2", max_batch=8)
    assert got.dtype == torch.uint8 and tuple(got.shape) == (F_, H_, W_, 3) and torch.equal(frames, keep)
    assert torch.equal(got, _compose(frames, res))                           # thick 1 and strip 4 are the defaults here
    assert model.calls == [(8, None)]                                        # 7 rows, filled up to max_batch
    # overlays appear on the segment's rows of track 0 and nowhere else
    plain = pred_func.render_scan(frames, res, model, evidence=False, layer="s2")
    assert model.calls == [(8, None)] and torch.equal(plain, _compose(frames, res, evidence=False))
    differs = (got != plain).any(-1)
    for f in range(F_):
        if 8 <= f <= 14:
            _, top, right, bottom, left = res["tracks"][0][f - 4]
            inside = torch.zeros((H_, W_), dtype=torch.bool)
            inside[top:bottom, left:right] = True
            assert differs[f].any() and not differs[f][~inside].any(), f
        else:
            assert not differs[f].any(), f
    assert torch.equal(pred_func.render_scan(frames, res, None, layer="s2"), plain)       # no model: no evidence
    # the timeline: lane 1 is red exactly on frames 8 ... 14; faceless frames carry it too
    low = got[23, H_ - 1].tolist()                                           # t = (24 x) // 64 is 8 ... 14 for x = 22 ... 39
    assert low[:22] == [[0x20] * 3] * 22 and low[22:40] == [[255, 0, 0]] * 18 and low[40:61] == [[0x20] * 3] * 21
    assert low[61:] == [[255] * 3] * 3                                       # the cursor of frame 23: (23 * 64) // 24 = 61
    assert got[23, H_ - 4, 56:61].tolist() == [[0x40] * 3] * 5               # frames 21 and 22: no crop
    assert got[23, H_ - 4, 0].tolist() != [0x40] * 3 and torch.equal(got[23, :H_ - 4], frames[23, :H_ - 4])


def test_render_scan_groups_sub_batches_eps_and_sink(on_the_cpu):
    frames, res = _scene()
    whole = pred_func.render_scan(frames, res, StandIn(), layer="s2", max_batch=8)
    model = StandIn()
    n = len(res["boxes"])
    eps = torch.arange(n, dtype=torch.float32)[:, None].expand(n, 4)
    assert torch.equal(pred_func.render_scan(frames, res, model, layer="s2", max_frames=5, max_batch=8, eps=eps), whole)
    # frames 8, 9 | 10 ... 14: crop rows 4, 5 | 6 ... 10, each call filled up to max_batch with its last row
    assert model.calls == [(8, [4.0, 5.0] + [5.0] * 6), (8, [6.0, 7.0, 8.0, 9.0, 10.0] + [10.0] * 3)]
    model = StandIn()
    assert torch.equal(pred_func.render_scan(frames, res, model, layer="s2", max_frames=7, max_batch=3, eps=eps), whole)
    assert model.calls == [(3, [4.0, 5.0, 6.0]), (3, [7.0, 8.0, 9.0]), (3, [10.0, 10.0, 10.0])]
    seen = []
    assert pred_func.render_scan(frames, res, StandIn(), layer="s2", max_frames=5, max_batch=8, sink=lambda g, s: seen.append((g, s.clone()))) is None
    assert [g for g, _ in seen] == [0, 5, 10, 15, 20] and [len(s) for _, s in seen] == [5, 5, 5, 5, 4]
    assert torch.equal(torch.cat([s for _, s in seen]), whole)


def test_render_scan_labels_thick_strip_lut_and_alpha(on_the_cpu):
    frames, res = _scene()
    res["persons"] = {"of_track": [5, 1000]}
    got = pred_func.render_scan(frames, res, StandIn(), label="person", layer="s2", max_batch=8)
    assert torch.equal(got, _compose(frames, res, names=[5, -1]))             # a number above 999 draws no tab
    assert not torch.equal(got, _compose(frames, res))
    assert torch.equal(pred_func.render_scan(frames, res, StandIn(), label=None, layer="s2", max_batch=8), _compose(frames, res, names=[-1, -1]))
    lut = au.frames_of((256, 3), 202)
    got = pred_func.render_scan(frames, res, StandIn(), layer="s2", thick=3, strip=0, lut=lut, alpha=1.0, max_batch=8)
    assert torch.equal(got, _compose(frames, res, thick=3, strip=0, lut=lut, alpha=1.0))
    assert torch.equal(pred_func.render_scan(frames, res, StandIn(), layer="s2", strip=9, max_batch=8), _compose(frames, res, strip=9))
    del res["persons"]
    with pytest.raises(ValueError, match="persons"):
        pred_func.render_scan(frames, res, StandIn(), label="person")


def test_render_scan_defaults_follow_the_frame_size(on_the_cpu):
    frames = au.frames_of((1, 480, 500, 3), 203)
    res = {"boxes": [(0, 10, 200, 100, 20)], "track_offsets": [0, 1], "frame_scores": torch.tensor([[1.0, 0.0]]), "segments": []}
    got = pred_func.render_scan(frames, res)
    lut = ou.jet_lut_ref()
    want = au.annotate_ref(frames, [0], [(0, 10, 200, 100, 20, au.pack(*lut[255].tolist()), 2, 0)],
                           torch.tensor([[au.pack(*lut[255].tolist())], [0x202020]]), 13)      # 480 // 240, 480 // 36
    assert torch.equal(got, want)


def test_render_scan_without_a_face_never_calls_the_model(on_the_cpu):
    frames = au.frames_of((7, 20, 30, 3), 204)

    class Never(torch.nn.Module):
        def parameters(self, recurse=True):
            return iter([torch.zeros(1)])

        def explain(self, *a, **k):
            raise AssertionError("the model was called")
    res = {"boxes": [], "track_offsets": [0], "frame_scores": torch.empty((0, 2)), "segments": []}
    got = pred_func.render_scan(frames, res, Never(), max_frames=3)
    tl = torch.tensor([[0x404040] * 7, [0x202020] * 7])
    assert torch.equal(got, au.annotate_ref(frames, list(range(7)), [], tl, 4)) and not torch.equal(got, frames)
    assert torch.equal(pred_func.render_scan(frames, res, Never(), strip=0), frames)
    # evidence=False: no call even with a segment
    frames, res = _scene()
    never = Never()
    never.net = "ed"
    assert torch.equal(pred_func.render_scan(frames, res, never, evidence=False), _compose(frames, res, evidence=False))


def test_render_scan_rejects_bad_input_before_anything_runs(monkeypatch):
    for name in ("face_crop_preprocess", "cam_overlay", "scan_annotate"):
        monkeypatch.setattr(_lib, name, lambda *a, **k: (_ for _ in ()).throw(AssertionError("something ran")))
    frames, res = _scene()
    for key in ("boxes", "track_offsets", "frame_scores", "segments"):
        with pytest.raises(ValueError, match="res must be the dict scan_frames returned"):
            pred_func.render_scan(frames, {k: v for k, v in res.items() if k != key})
    with pytest.raises(ValueError, match="res must be the dict"):
        pred_func.render_scan(frames, [res])
    with pytest.raises(ValueError, match="crop row 26 is not"):
        pred_func.render_scan(frames, dict(res, boxes=res["boxes"][:-1] + [(F_, 20, 62, 44, 30)]))
    with pytest.raises(ValueError, match="lies outside its 48x64 frame"):
        pred_func.render_scan(frames, dict(res, boxes=res["boxes"][:-1] + [(9, 20, 65, 44, 30)]))
    with pytest.raises(ValueError, match="unknown label"):
        pred_func.render_scan(frames, res, label="name")
    with pytest.raises(ValueError, match="unknown map"):
        pred_func.render_scan(frames, res, which="both")
    with pytest.raises(ValueError, match="track_offsets"):
        pred_func.render_scan(frames, dict(res, track_offsets=[0, 17]))
    with pytest.raises(ValueError, match="frame_scores"):
        pred_func.render_scan(frames, dict(res, frame_scores=res["frame_scores"][:5]))
    with pytest.raises(ValueError, match="eps holds 3 rows"):
        pred_func.render_scan(frames, res, StandIn(), eps=torch.zeros((3, 4)))
    for kw in (dict(thick=0), dict(thick=17), dict(strip=1), dict(strip=H_ + 1), dict(max_frames=0), dict(max_batch=0)):
        with pytest.raises(ValueError):
            pred_func.render_scan(frames, res, **kw)
    with pytest.raises(_lib.GenConViTHipError):
        pred_func.render_scan(frames.float(), res)


def test_render_video_reads_once_scans_and_renders(on_the_cpu, monkeypatch):
    frames, res = _scene()
    reads, scans = [], []

    def read(vid, select):
        reads.append(vid)
        index = list(select(100))
        return frames.numpy()[:len(index)], index

    def scan(fr, model, **kw):
        scans.append((fr.shape, kw))
        return dict(res)
    monkeypatch.setattr(pred_func, "_read_frames", read)
    monkeypatch.setattr(pred_func, "scan_frames", scan)
    model = StandIn()
    got, rendered = pred_func.render_video("clip.mp4", model, every=3, max_frames=F_, scan={"window": 4}, layer="s2", thick=2, max_batch=8)
    assert reads == ["clip.mp4"] and scans == [((F_, H_, W_, 3), {"window": 4})]
    assert got["frame_index"] == list(range(0, 3 * F_, 3)) and got["segments"] == res["segments"]
    assert torch.equal(rendered, _compose(frames, res, thick=2)) and model.calls == [(8, None)]
    with pytest.raises(ValueError):
        pred_func.render_video("clip.mp4", model, every=0)
