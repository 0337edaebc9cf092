"""The YUV 4:2:0 arithmetic of gcv_yuv420_to_rgb / gcv_rgb_to_yuv420 as tests/yuvutil.py restates it (no GPU): the coefficient
literals against their derivation, the integer conversion against the real-number formula over every (Y, U, V), the exact
points (grey, white), the two layouts, the format's own round-trip loss, and the argument checks of ``pred_func.YUV420``,
``read_yuv420`` and ``render_scan(out=...)``."""
import io
import itertools
import os
import re

import numpy as np
import pytest
import torch

from genconvit_amd import _lib
from genconvit_amd.model import pred_func
from tests import yuvutil as yu

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KEYS = list(itertools.product(yu.MATRICES, yu.RANGES))
# the worst |c' - c| of a flat colour c through RGB -> YUV -> RGB over all 2^24 colours: what the 8-bit format loses, whatever
# converts it (DESIGN.md §4.12 quotes these)
ROUND_TRIP_WORST = {("bt601", False): 2, ("bt601", True): 1, ("bt709", False): 2, ("bt709", True): 1}


@pytest.mark.parametrize("matrix,full", KEYS)
def test_the_literals_are_the_derivation(matrix, full):
    assert yu.COEF_IN[(matrix, full)] == yu.derive_in(matrix, full)
    assert yu.COEF_OUT[(matrix, full)] == yu.derive_out(matrix, full)
    oy, luma, urow, vrow = yu.COEF_OUT[(matrix, full)]
    assert sum(urow) == 0 and sum(vrow) == 0 and sum(luma) == (16384 if full else 14071)


def test_the_kernel_source_and_the_header_hold_the_same_literals():
    src = open(os.path.join(REPO, "genconvit_amd", "csrc", "yuv.hip")).read()
    hdr = open(os.path.join(REPO, "include", "genconvit_hip.h")).read()
    flat = lambda row: [v for part in row for v in (part if isinstance(part, tuple) else (part,))]
    for key in KEYS:
        for row in (flat(yu.COEF_IN[key]), flat(yu.COEF_OUT[key])):
            assert "{" + ", ".join(str(v) for v in row) + "}" in src, (key, row)
            assert re.sub(r"[;,]", "", " ".join(str(v) for v in row)) in re.sub(r"[;,]", "", hdr), (key, row)
    assert re.search(r"int gcv_yuv420_to_rgb\(const void\* yuv_u8,", hdr) and re.search(r"int gcv_rgb_to_yuv420\(", hdr)
    assert len(_lib.SIGNATURES["gcv_yuv420_to_rgb"][1]) == 9 and len(_lib.SIGNATURES["gcv_rgb_to_yuv420"][1]) == 9


@pytest.mark.parametrize("matrix,full", KEYS)
def test_every_yuv_triple_is_within_one_of_the_real_formula(matrix, full):
    """14-bit coefficients are off by at most 2^-15 each, the inputs are at most 255 and there are three terms: the integer
    value is within 0.03 of the real one before rounding, so the rounded bytes differ by at most 1.  A condition, not a
    measurement; ``sample_rgb`` is the arithmetic ``to_rgb_ref`` applies to the samples it gathers (checked below)."""
    u, v = np.meshgrid(np.arange(256), np.arange(256), indexing="ij")
    worst = 0
    for y in range(256):
        yy = np.full_like(u, y)
        for got, real in zip(yu.sample_rgb(yy, u, v, matrix, full), yu.float_rgb(yy, u, v, matrix, full)):
            worst = max(worst, int(np.abs(got - np.clip(np.rint(real), 0, 255)).max()))
    print(f"\n{matrix} full_range={full}: worst |integer - real| over 2^24 triples = {worst}")
    assert worst <= 1


@pytest.mark.parametrize("layout", yu.LAYOUTS)
def test_the_frame_restatements_apply_the_sample_arithmetic(layout):
    for matrix, full in KEYS:
        yuv = yu.case_in("table", layout)
        y, u, v = (p.astype(np.int64) for p in yu.planes(yuv, layout))
        up = lambda c: np.repeat(np.repeat(c, 2, 1), 2, 2)
        want = np.stack(yu.sample_rgb(y, up(u), up(v), matrix, full), -1).astype(np.uint8)
        assert np.array_equal(yu.to_rgb_ref(yuv, layout, matrix, full), want)
        rgb = yu.case_out("flat")
        fy, fu, fv = yu.flat_yuv(rgb[:, 0, 0], matrix, full)
        py, pu, pv = yu.planes(yu.to_yuv_ref(rgb, layout, matrix, full), layout)
        assert (py == fy[:, None, None]).all() and (pu == fu[:, None, None]).all() and (pv == fv[:, None, None]).all()


@pytest.mark.parametrize("matrix,full", KEYS)
def test_grey_and_white_are_exact(matrix, full):
    grey = np.repeat(np.arange(256)[:, None], 3, 1)
    y, u, v = yu.flat_yuv(grey, matrix, full)
    assert (u == 128).all() and (v == 128).all()
    assert y[255] == (255 if full else 235) and y[0] == (0 if full else 16)
    frame = np.full((1, 4, 6, 3), 255, dtype=np.uint8)
    for layout in yu.LAYOUTS:
        py, pu, pv = yu.planes(yu.to_yuv_ref(frame, layout, matrix, full), layout)
        assert (py == (255 if full else 235)).all() and (pu == 128).all() and (pv == 128).all()
    back = yu.sample_rgb(y, u, v, matrix, full)
    assert all(int(np.abs(c - np.arange(256)).max()) <= 1 for c in back) and all(c[255] == 255 and c[0] == 0 for c in back)


def test_i420_and_nv12_hold_the_same_samples():
    for name in yu.SMALL_OUT:
        rgb = yu.case_out(name)
        for matrix, full in KEYS:
            a, b = (yu.planes(yu.to_yuv_ref(rgb, lay, matrix, full), lay) for lay in yu.LAYOUTS)
            assert all(np.array_equal(p, q) for p, q in zip(a, b))
    yuv = yu.case_in("rand_6x10", "i420")
    swapped = yu.pack(*yu.planes(yuv, "i420"), "nv12")
    assert not np.array_equal(yuv, swapped)
    assert np.array_equal(yu.to_rgb_ref(yuv, "i420"), yu.to_rgb_ref(swapped, "nv12"))
    for lay in yu.LAYOUTS:
        assert np.array_equal(yu.pack(*yu.planes(yuv, lay), lay), yuv)


@pytest.mark.parametrize("matrix,full", KEYS)
def test_the_flat_colour_round_trip_of_the_format(matrix, full):
    g, b = np.meshgrid(np.arange(256), np.arange(256), indexing="ij")
    worst = 0
    for r in range(256):
        rgb = np.stack([np.full_like(g, r), g, b], -1)
        back = np.stack(yu.sample_rgb(*yu.flat_yuv(rgb, matrix, full), matrix, full), -1)
        worst = max(worst, int(np.abs(back - rgb).max()))
    assert worst == ROUND_TRIP_WORST[(matrix, full)]
    design = open(os.path.join(REPO, "DESIGN.md")).read()
    assert f"{matrix} {'full' if full else 'limited'} {worst}" in design


def test_the_cases_are_what_the_issue_lists():
    strides = [yu.case_in(n, "i420")[0].size for n in yu.RANDOM]
    # a frame is a multiple of 6 bytes, so packed frames start at 0 or 2 mod 4: both occur (odd starts: test_yuv_gpu's views)
    assert strides == [6, 18, 90, 96, 510] and {(k * s) % 4 for s in strides for k in range(3)} == {0, 2}
    assert {s % 8 for s in strides} == {6, 2, 0} and {int(n.split("x")[1]) % 8 for n in yu.RANDOM} == {2, 6, 0}
    assert all(yu.case_in(n, "i420").shape[0] == 3 for n in yu.RANDOM)
    y, u, v = yu.planes(yu.case_in("table", "nv12"), "nv12")
    triples = {(int(a), int(b), int(c)) for a, b, c in zip(y[0, ::2, ::2].ravel(), u.ravel(), v.ravel())}
    assert triples == set(itertools.product(range(256), yu.TABLE_UV, yu.TABLE_UV))
    assert yu.case_in("720p", "i420").shape == (2, 1080, 1280) and yu.case_out("720p").shape == (2, 720, 1280, 3)
    blocks = yu.case_out("steps").reshape(16, 2, 16, 2, 3).transpose(0, 2, 1, 3, 4).reshape(256, 4, 3)
    assert all(len({tuple(p) for p in blk}) == 4 for blk in blocks.tolist())


def test_the_build_refuses_the_fused_shift_and_pack(tmp_path):
    """csrc/isa_report.py check 4, on a hand-written listing: the instruction hipcc forms from clip(a >> n) | clip(b >> n) << 8,
    whose upper half the first yuv.hip relied on and got wrong bytes for; and yuv.hip clips before it shifts."""
    import importlib.util
    spec_ = importlib.util.spec_from_file_location("isa_report", os.path.join(REPO, "genconvit_amd", "csrc", "isa_report.py"))
    isa = importlib.util.module_from_spec(spec_)
    spec_.loader.exec_module(isa)
    listing = ("_Z4testv:\n{}\ts_endpgm\n.Lfunc_end0:\n  - .agpr_count:     0\n    .group_segment_fixed_size: 0\n"
               "    .name:           _Z4testv\n    .private_segment_fixed_size: 0\n    .sgpr_count:     10\n    .vgpr_count:     8\n"
               "    .vgpr_spill_count: 0\n")
    f = tmp_path / "k.s"
    f.write_text(listing.format("\tv_ashr_pk_u8_i32 v16, v16, v17, 14\n\tv_or3_b32 v21, v16, v15, v18\n"))
    got = isa.check_file(str(f))
    assert len(got) == 1 and "check 4" in got[0], got
    f.write_text(listing.format("\tv_med3_i32 v16, v16, 0, v27\n\tv_ashrrev_i32_e32 v16, 14, v16\n"))
    assert isa.check_file(str(f)) == []
    src = open(os.path.join(REPO, "genconvit_amd", "csrc", "yuv.hip")).read()
    assert src.count("yuv_clip14(l") == 6                  # the six channels of a pixel pair


# ------------------------------------------------------------------------------------- the public surface, off the device
def test_yuv420_describes_its_frames():
    data = yu.case_in("rand_6x10", "i420")
    for given in (data, torch.as_tensor(data)):
        fr = pred_func.YUV420(given, "nv12", "bt601", True)
        assert fr.shape == (3, 6, 10, 3) and len(fr) == 3 and not fr.is_cuda and fr.device == torch.device("cpu")
        assert (fr.layout, fr.matrix, fr.full_range) == ("nv12", "bt601", True)
        assert pred_func._as_frames("x", fr) is fr and not pred_func._resident(fr)
    assert pred_func.YUV420(data[:0]).shape == (0, 6, 10, 3)


@pytest.mark.parametrize("bad", [np.zeros((2, 9, 10), np.float32), np.zeros((9, 10), np.uint8), np.zeros((2, 10, 10), np.uint8),
                                 np.zeros((2, 9, 5), np.uint8), np.zeros((2, 0, 4), np.uint8), np.zeros((2, 3, 0), np.uint8),
                                 np.zeros((2, 6, 10, 3), np.uint8)])
def test_yuv420_refuses_bad_shapes(bad):
    with pytest.raises(_lib.GenConViTHipError, match="YUV420"):
        pred_func.YUV420(bad)


def test_yuv420_refuses_unknown_names():
    data = np.zeros((1, 3, 2), np.uint8)
    for kw in (dict(layout="yv12"), dict(matrix="bt2020"), dict(layout=None)):
        with pytest.raises(_lib.GenConViTHipError, match="YUV420: unknown"):
            pred_func.YUV420(data, **kw)
    with pytest.raises(_lib.GenConViTHipError, match="frames must be uint8"):
        pred_func._as_frames("x", data)


def test_the_bindings_refuse_before_they_need_a_device():
    good = torch.zeros((2, 9, 10), dtype=torch.uint8)
    for bad, kw in ((good.float(), {}), (good[0], {}), (torch.zeros((2, 10, 10), dtype=torch.uint8), {}),
                    (torch.zeros((2, 9, 5), dtype=torch.uint8), {}), (good.numpy(), {}), (good, dict(layout="nv21")),
                    (good, dict(matrix="709")), (good, {})):                 # the last: a host tensor
        with pytest.raises(_lib.GenConViTHipError, match="yuv420_to_rgb"):
            _lib.yuv420_to_rgb(bad, **kw)
    rgb = torch.zeros((2, 6, 10, 3), dtype=torch.uint8)
    for bad, kw in ((rgb.float(), {}), (rgb[0], {}), (rgb[:, :5], {}), (rgb[:, :, :3], {}), (rgb, dict(layout="yuv")),
                    (rgb, dict(matrix=1)), (rgb, {})):
        with pytest.raises(_lib.GenConViTHipError, match="rgb_to_yuv420"):
            _lib.rgb_to_yuv420(bad, **kw)


def test_read_yuv420(tmp_path):
    data = yu.case_in("rand_6x10", "i420")
    raw = data.tobytes()
    path = tmp_path / "clip.yuv"
    path.write_bytes(raw)
    for src in (str(path), path, io.BytesIO(raw)):
        fr = pred_func.read_yuv420(src, 6, 10, "nv12", matrix="bt601", full_range=True)
        assert isinstance(fr, pred_func.YUV420) and fr.shape == (3, 6, 10, 3) and np.array_equal(fr.data.numpy(), data)
        assert (fr.layout, fr.matrix, fr.full_range) == ("nv12", "bt601", True)
    assert pred_func.read_yuv420(str(path), 6, 10, max_frames=2).shape == (2, 6, 10, 3)
    assert pred_func.read_yuv420(io.BytesIO(raw), 6, 10, max_frames=2).shape == (2, 6, 10, 3)
    assert pred_func.read_yuv420(io.BytesIO(raw), 6, 10, max_frames=7).shape == (3, 6, 10, 3)
    assert pred_func.read_yuv420(io.BytesIO(b""), 6, 10).shape == (0, 6, 10, 3)

    class Dribble(io.BytesIO):                              # a pipe that hands over 7 bytes at a time
        def read(self, n=-1):
            return super().read(7 if n < 0 else min(n, 7))
    assert np.array_equal(pred_func.read_yuv420(Dribble(raw), 6, 10).data.numpy(), data)
    for src in (io.BytesIO(raw[:-1]), io.BytesIO(raw + b"x")):
        with pytest.raises(_lib.GenConViTHipError, match="partial"):
            pred_func.read_yuv420(src, 6, 10)
    (tmp_path / "cut.yuv").write_bytes(raw[:100])
    with pytest.raises(_lib.GenConViTHipError, match="partial"):
        pred_func.read_yuv420(str(tmp_path / "cut.yuv"), 6, 10)
    for h, w in ((5, 10), (6, 9), (0, 10), (6.0, 10)):
        with pytest.raises(_lib.GenConViTHipError, match="read_yuv420: H"):
            pred_func.read_yuv420(io.BytesIO(raw), h, w)
    with pytest.raises(_lib.GenConViTHipError, match="max_frames"):
        pred_func.read_yuv420(io.BytesIO(raw), 6, 10, max_frames=-1)
    with pytest.raises(_lib.GenConViTHipError, match="unknown layout"):
        pred_func.read_yuv420(io.BytesIO(raw), 6, 10, "yv12")


def test_render_scan_checks_out_before_anything_runs():
    frames = np.zeros((2, 6, 10, 3), np.uint8)
    with pytest.raises(ValueError, match="unknown out 'yuv'"):
        pred_func.render_scan(frames, {}, out="yuv")
    with pytest.raises(ValueError, match="unknown out_matrix"):
        pred_func.render_scan(frames, {}, out="nv12", out_matrix="bt2020")
    for odd in (np.zeros((2, 5, 10, 3), np.uint8), np.zeros((2, 6, 9, 3), np.uint8)):
        with pytest.raises(ValueError, match="even height and width"):
            pred_func.render_scan(odd, {}, out="i420")
    with pytest.raises(ValueError, match="res must be the dict"):                # a good out: the next check speaks
        pred_func.render_scan(frames, {}, out="i420")
    with pytest.raises(ValueError, match="res must be the dict"):
        pred_func.render_scan(pred_func.YUV420(np.zeros((2, 9, 10), np.uint8)), {}, out="nv12", out_matrix="ignored")
