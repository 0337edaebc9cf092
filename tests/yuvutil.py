"""CPU restatement, in numpy, of the arithmetic of gcv_yuv420_to_rgb and gcv_rgb_to_yuv420 (include/genconvit_hip.h;
csrc/yuv.hip), written from the header's statement and not from the kernels: ``to_rgb_ref`` and
``to_yuv_ref`` in int64, both layouts, with the coefficient literals, their derivation from (Kr, Kb) in exact fractions,
the cases the tests run, and ``DEFECTS_IN`` / ``DEFECTS_OUT``: the same restatements with one defect planted each, and for
every defect the cases that must tell it from the right one (tests/test_yuv_sensitivity_cpu.py)."""
import functools
import itertools
import math
from fractions import Fraction

import numpy as np

LAYOUTS = ("i420", "nv12")
MATRICES = ("bt601", "bt709")
RANGES = (False, True)                                     # full_range
KR_KB = {"bt601": (Fraction(299, 1000), Fraction(114, 1000)), "bt709": (Fraction(2126, 10000), Fraction(722, 10000))}

# (matrix, full_range) -> (oy, cy, crv, cgu, cgv, cbu): R = cy y' + crv v', G = cy y' + cgu u' + cgv v', B = cy y' + cbu u'
COEF_IN = {
    ("bt601", False): (16, 19077, 26149, -6419, -13320, 33050),
    ("bt601", True): (0, 16384, 22970, -5638, -11700, 29032),
    ("bt709", False): (16, 19077, 29372, -3494, -8731, 34610),
    ("bt709", True): (0, 16384, 25802, -3069, -7670, 30402),
}
# (matrix, full_range) -> (oy, (ar, ag, ab), (ur, ug, ub), (vr, vg, vb))
COEF_OUT = {
    ("bt601", False): (16, (4207, 8260, 1604), (-2428, -4768, 7196), (7196, -6026, -1170)),
    ("bt601", True): (0, (4899, 9617, 1868), (-2765, -5427, 8192), (8192, -6860, -1332)),
    ("bt709", False): (16, (2991, 10064, 1016), (-1649, -5547, 7196), (7196, -6536, -660)),
    ("bt709", True): (0, (3483, 11718, 1183), (-1877, -6315, 8192), (8192, -7441, -751)),
}


def _rnd(q):
    """round half up of an exact fraction"""
    return math.floor(q + Fraction(1, 2))


def derive_in(matrix, full_range):
    """``COEF_IN``'s row from (Kr, Kb): every real coefficient times 2^14, rounded"""
    kr, kb = KR_KB[matrix]
    kg = 1 - kr - kb
    ky = Fraction(1) if full_range else Fraction(255, 219)
    kc = Fraction(1) if full_range else Fraction(255, 224)
    one = 1 << 14
    return (0 if full_range else 16, _rnd(ky * one), _rnd(kc * 2 * (1 - kr) * one), _rnd(-kc * 2 * (1 - kb) * kb / kg * one),
            _rnd(-kc * 2 * (1 - kr) * kr / kg * one), _rnd(kc * 2 * (1 - kb) * one))


def derive_out(matrix, full_range):
    """``COEF_OUT``'s row from (Kr, Kb): luma's green makes white exact, chroma's green makes each row sum to 0"""
    kr, kb = KR_KB[matrix]
    s = Fraction(1) if full_range else Fraction(219, 255)
    t = Fraction(1) if full_range else Fraction(224, 255)
    one = 1 << 14
    ar, ab = _rnd(kr * s * one), _rnd(kb * s * one)
    ur, ub = _rnd(-kr / (2 * (1 - kb)) * t * one), _rnd((1 - kb) / (2 * (1 - kb)) * t * one)
    vr, vb = _rnd((1 - kr) / (2 * (1 - kr)) * t * one), _rnd(-kb / (2 * (1 - kr)) * t * one)
    return (0 if full_range else 16, (ar, _rnd(s * one) - ar - ab, ab), (ur, -ur - ub, ub), (vr, -vr - vb, vb))


def float_rgb(y, u, v, matrix, full_range):
    """the real-number formula, float64, before rounding and clipping: what the 14-bit integers approximate"""
    kr, kb = (float(k) for k in KR_KB[matrix])
    kg = 1.0 - kr - kb
    ky, kc = (1.0, 1.0) if full_range else (255.0 / 219.0, 255.0 / 224.0)
    yy = ky * (np.asarray(y, dtype=np.float64) - (0.0 if full_range else 16.0))
    uu, vv = np.asarray(u, dtype=np.float64) - 128.0, np.asarray(v, dtype=np.float64) - 128.0
    return (yy + kc * 2 * (1 - kr) * vv, yy - kc * 2 * (1 - kb) * kb / kg * uu - kc * 2 * (1 - kr) * kr / kg * vv,
            yy + kc * 2 * (1 - kb) * uu)


def geometry(yuv):
    f, rows, w = yuv.shape
    h = rows * 2 // 3
    assert yuv.dtype == np.uint8 and h * 3 == rows * 2 and h % 2 == 0 and w % 2 == 0 and h >= 2 and w >= 2
    return f, h, w


def planes(yuv, layout):
    """(Y (F,H,W), U (F,H/2,W/2), V (F,H/2,W/2)) of a (F, 3H/2, W) buffer: the layout as the header words it"""
    f, h, w = geometry(yuv)
    flat = yuv.reshape(f, -1)
    y = flat[:, :h * w].reshape(f, h, w)
    if layout == "i420":
        u = flat[:, h * w:h * w + h * w // 4].reshape(f, h // 2, w // 2)
        v = flat[:, h * w + h * w // 4:].reshape(f, h // 2, w // 2)
    else:
        uv = flat[:, h * w:].reshape(f, h // 2, w // 2, 2)
        u, v = uv[..., 0], uv[..., 1]
    return y, u, v


def pack(y, u, v, layout):
    """the inverse of ``planes``"""
    f, h, w = y.shape
    if layout == "i420":
        flat = np.concatenate([y.reshape(f, -1), u.reshape(f, -1), v.reshape(f, -1)], axis=1)
    else:
        flat = np.concatenate([y.reshape(f, -1), np.stack([u, v], axis=-1).reshape(f, -1)], axis=1)
    return np.ascontiguousarray(flat.astype(np.uint8).reshape(f, 3 * h // 2, w))


def _rgb_arith(y, u, v, coef, half=8192, clip=None):
    """[R, G, B] of int64 samples Y and U - 128, V - 128: the header's integer arithmetic, which ``to_rgb_with`` applies to
    the samples it gathered (``half``, ``clip``: its arithmetic defects)"""
    oy, cy, crv, cgu, cgv, cbu = coef
    lum = cy * (y - oy) + half
    chans = [(lum + crv * v) >> 14, (lum + cgu * u + cgv * v) >> 14, (lum + cbu * u) >> 14]
    if clip == "no_clip":
        return [c & 255 for c in chans]
    if clip == "no_low_clip":
        return [np.minimum(c, 255) & 255 for c in chans]
    return [np.clip(c, 0, 255) for c in chans]


def sample_rgb(y, u, v, matrix, full_range):
    """[R, G, B] of arrays of samples Y, U, V (0 ... 255), without a frame around them: ``to_rgb_ref``'s own arithmetic"""
    return _rgb_arith(np.asarray(y, dtype=np.int64), np.asarray(u, dtype=np.int64) - 128, np.asarray(v, dtype=np.int64) - 128,
                      COEF_IN[(matrix, full_range)])


def _yuv_arith(p, s, coef, oy_on=True, half=32768, clip=True):
    """Y of int64 pixels ``p`` (..., 3) and U, V of block sums ``s`` (..., 3): the header's integer arithmetic, which
    ``to_yuv_with`` applies to the pixels and the sums it took"""
    oy, (ar, ag, ab), urow, vrow = coef
    y = (oy if oy_on else 0) + ((ar * p[..., 0] + ag * p[..., 1] + ab * p[..., 2] + 8192) >> 14)
    chroma = [128 + ((row[0] * s[..., 0] + row[1] * s[..., 1] + row[2] * s[..., 2] + half) >> 16) for row in (urow, vrow)]
    u, v = [np.clip(c, 0, 255) if clip else c & 255 for c in chroma]
    return y, u, v


def flat_yuv(rgb, matrix, full_range):
    """(Y, U, V) of blocks that hold one colour each, ``rgb`` (..., 3): the block sum is four times the pixel"""
    p = np.asarray(rgb, dtype=np.int64)
    return _yuv_arith(p, 4 * p, COEF_OUT[(matrix, full_range)])


def to_rgb_with(yuv, layout="i420", matrix="bt709", full_range=False, defect=None):
    """gcv_yuv420_to_rgb on the CPU with one of ``DEFECTS_IN`` planted (None: the header's arithmetic).  The samples are
    gathered from the flat byte buffer by index, as a kernel addresses them, so that addressing defects can be stated;
    an index a defect pushes past the buffer wraps around."""
    assert defect is None or defect in DEFECTS_IN, defect
    nf, h, w = geometry(yuv)
    hw = h * w
    buf = yuv.reshape(-1).astype(np.int64)
    f, y, x = np.indices((nf, h, w), dtype=np.int64)
    base = f * (hw if defect == "frame_stride_hw" else 3 * hw // 2)
    cy_ = y if defect == "chroma_row_y" else y // 2
    cx_ = x if defect == "chroma_col_x" else x // 2
    if layout == "i420" or defect == "nv12_as_i420":
        iu = base + hw + cy_ * (w if defect == "u_stride_w" else w // 2) + cx_
        iv = base + hw + (0 if defect == "v_at_u" else hw // 4) + cy_ * (w // 2) + cx_
    else:
        iu = base + hw + cy_ * w + 2 * cx_
        iv = iu + 1
        if defect == "nv21":
            iu, iv = iv, iu
    yv = buf.take(base + (y & ~1 if defect == "lower_row_upper_y" else y) * w + x, mode="wrap")
    u, v = buf.take(iu, mode="wrap") - 128, buf.take(iv, mode="wrap") - 128
    if defect == "uv_swap":
        u, v = v, u
    oy, cy, crv, cgu, cgv, cbu = COEF_IN[("bt601" if defect == "bt601_under_bt709" else matrix, full_range)]
    if defect == "oy_kept":
        oy = 16
    if defect == "oy_dropped":
        oy = 0
    if defect == "g_v_sign":
        cgv = -cgv
    chans = _rgb_arith(yv, u, v, (oy, cy, crv, cgu, cgv, cbu), 0 if defect == "no_round" else 8192,
                       defect if defect in ("no_clip", "no_low_clip") else None)
    rgb = np.stack(chans, axis=-1).astype(np.uint8)
    if defect == "drop_tail" and w % 8:
        rgb[:, :, w - w % 8:] = 0
    return rgb


def to_yuv_with(rgb, layout="i420", matrix="bt709", full_range=False, defect=None):
    """gcv_rgb_to_yuv420 on the CPU with one of ``DEFECTS_OUT`` planted (None: the header's arithmetic)."""
    assert defect is None or defect in DEFECTS_OUT, defect
    nf, h, w, _ = rgb.shape
    assert rgb.dtype == np.uint8 and h % 2 == 0 and w % 2 == 0 and h >= 2 and w >= 2
    p = rgb.astype(np.int64)
    if defect == "rb_swap":
        p = p[..., ::-1]
    blocks = p.reshape(nf, h // 2, 2, w // 2, 2, 3)
    s = 4 * blocks[:, :, 0, :, 0] if defect == "topleft" else blocks.sum(axis=(2, 4))
    y, u, v = _yuv_arith(p, s, COEF_OUT[(matrix, full_range)], defect != "no_oy", 0 if defect == "no_round_c" else 32768,
                         defect != "no_clip_c")
    if defect == "odd_rows_y":
        y[:, 1::2] = 0
    if defect == "drop_tail" and w % 8:
        y[:, :, w - w % 8:] = 0
        u[:, :, (w - w % 8) // 2:] = 0
        v[:, :, (w - w % 8) // 2:] = 0
    if defect == "v_at_u":
        u, v = v, np.zeros_like(v)
    if defect == "nv21" and layout == "nv12":
        u, v = v, u
    return pack(y, u, v, layout)


def to_rgb_ref(yuv, layout="i420", matrix="bt709", full_range=False):
    """gcv_yuv420_to_rgb on the CPU: uint8 (F, 3H/2, W) -> uint8 (F,H,W,3)"""
    return to_rgb_with(yuv, layout, matrix, full_range)


def to_yuv_ref(rgb, layout="i420", matrix="bt709", full_range=False):
    """gcv_rgb_to_yuv420 on the CPU: uint8 (F,H,W,3) -> uint8 (F, 3H/2, W)"""
    return to_yuv_with(rgb, layout, matrix, full_range)


# ---------------------------------------------------------------------------------------------------------- the cases
RANDOM_SIZES = ((2, 2), (2, 6), (6, 10), (4, 16), (10, 34))      # frame strides 6, 18, 90, 96 and 510 bytes
TABLE_UV = (0, 16, 128, 240, 255)
FLAT_IN = [(y, u, v) for y in (0, 16, 235, 255)
           for u, v in ((0, 0), (0, 255), (255, 0), (255, 255), (128, 128), (16, 240), (240, 16))]
FLAT_OUT = [(0, 0, 0), (255, 0, 0), (0, 255, 0), (0, 0, 255), (255, 255, 0), (255, 0, 255), (0, 255, 255), (255, 255, 255),
            (128, 128, 128), (16, 16, 16), (235, 235, 235)]


def _random(seed, shape):
    return np.random.default_rng(seed).integers(0, 256, size=shape, dtype=np.uint8)


def _table(layout):
    """every Y against U, V in TABLE_UV^2, one triple per 2x2 block: 6400 blocks as 80 x 80, one frame of 160 x 160"""
    yy, uv = np.meshgrid(np.arange(256), np.arange(25), indexing="ij")
    y, u, v = yy.reshape(80, 80), np.asarray(TABLE_UV)[uv // 5].reshape(80, 80), np.asarray(TABLE_UV)[uv % 5].reshape(80, 80)
    return pack(np.repeat(np.repeat(y, 2, 0), 2, 1)[None], u[None], v[None], layout)


def _flat_in(layout):
    """one flat 4 x 8 frame per entry of FLAT_IN"""
    t = np.asarray(FLAT_IN)
    ones = np.ones((len(t), 4, 8), dtype=np.int64)
    return pack(ones * t[:, 0, None, None], ones[:, :2, :4] * t[:, 1, None, None], ones[:, :2, :4] * t[:, 2, None, None], layout)


def _steps():
    """2x2 blocks of four different pixels whose chroma accumulator br Sr + bg Sg + bb Sb + 32768 lies within 600 of a
    multiple of 65536, below it or above: 32 of each side for the U row of each of the four tables, 256 blocks in all as
    one frame of 32 x 32.  600 is below the smallest non-zero coefficient, so one grey level in one channel of one pixel
    moves such a block across the step."""
    cand = _random(77, (200000, 2, 2, 3))
    distinct = np.asarray([len({tuple(px) for px in b.reshape(4, 3)}) == 4 for b in cand[:20000]])
    cand = cand[:20000][distinct]
    s = cand.astype(np.int64).sum(axis=(1, 2))
    picked = []
    for key in itertools.product(MATRICES, RANGES):
        ur, ug, ub = COEF_OUT[key][2]
        res = (ur * s[:, 0] + ug * s[:, 1] + ub * s[:, 2] + 32768) % 65536
        below, above = np.flatnonzero(res >= 65536 - 600)[:32], np.flatnonzero(res < 600)[:32]
        assert len(below) == 32 and len(above) == 32
        picked += [below, above]
    blocks = cand[np.concatenate(picked)].reshape(16, 16, 2, 2, 3)
    return np.ascontiguousarray(blocks.transpose(0, 2, 1, 3, 4).reshape(1, 32, 32, 3))


@functools.lru_cache(maxsize=None)
def case_in(name, layout):
    """the YUV input of a case: uint8 (F, 3H/2, W).  The random cases hold the same bytes for both layouts."""
    if name == "table":
        return _table(layout)
    if name == "flat":
        return _flat_in(layout)
    if name == "720p":
        return _random(720, (2, 1080, 1280))
    h, w = (int(v) for v in name.split("_")[1].split("x"))
    return _random(1000 * h + w, (3, 3 * h // 2, w))


@functools.lru_cache(maxsize=None)
def case_out(name):
    """the RGB input of a case: uint8 (F,H,W,3)"""
    if name == "flat":
        return np.ascontiguousarray(np.broadcast_to(np.asarray(FLAT_OUT, dtype=np.uint8)[:, None, None, :], (len(FLAT_OUT), 4, 8, 3)))
    if name == "steps":
        return _steps()
    if name == "720p":
        return _random(721, (2, 720, 1280, 3))
    h, w = (int(v) for v in name.split("_")[1].split("x"))
    return _random(2000 * h + w, (3, h, w, 3))


RANDOM = tuple(f"rand_{h}x{w}" for h, w in RANDOM_SIZES)
SMALL_IN = RANDOM + ("table", "flat")
SMALL_OUT = RANDOM + ("flat", "steps")
CASES_IN = SMALL_IN + ("720p",)
CASES_OUT = SMALL_OUT + ("720p",)
ODD_WIDTH = tuple(f"rand_{h}x{w}" for h, w in RANDOM_SIZES if w % 8)


def _where(cases, layouts=LAYOUTS, matrices=MATRICES, ranges=RANGES):
    return tuple(itertools.product(cases, layouts, matrices, ranges))


# defect -> (what is wrong, the (case, layout, matrix, full_range) that must each catch it)
DEFECTS_IN = {
    "uv_swap": ("U and V swapped", _where(RANDOM + ("table",))),
    "nv21": ("nv12 read as nv21", _where(RANDOM + ("table",), ("nv12",))),
    "nv12_as_i420": ("nv12 read as i420", _where(RANDOM[1:] + ("table",), ("nv12",))),
    "chroma_row_y": ("chroma row y instead of y / 2", _where(RANDOM + ("table",))),
    "chroma_col_x": ("chroma column x instead of x / 2", _where(RANDOM + ("table",))),
    "u_stride_w": ("U-plane rows strided by W instead of W / 2", _where(RANDOM[2:] + ("table",), ("i420",))),
    "v_at_u": ("V plane at the U plane's offset", _where(RANDOM + ("table",), ("i420",))),
    "frame_stride_hw": ("frame stride H W", _where(RANDOM + ("flat",))),
    "no_round": ("rounding term missing", _where(RANDOM + ("table",))),
    "no_clip": ("no clip: the byte wraps", _where(RANDOM + ("table", "flat"))),
    "no_low_clip": ("low clip missing", _where(RANDOM[1:] + ("table", "flat"))),
    "oy_kept": ("the limited-range 16 kept under full_range", _where(RANDOM + ("table", "flat"), ranges=(True,))),
    "oy_dropped": ("the limited-range 16 dropped without full_range", _where(RANDOM + ("table", "flat"), ranges=(False,))),
    "bt601_under_bt709": ("bt601 table under bt709", _where(RANDOM + ("table", "flat"), matrices=("bt709",))),
    "lower_row_upper_y": ("the lower row of a pair given the upper row's Y", _where(RANDOM)),
    "drop_tail": ("last W % 8 columns dropped", _where(ODD_WIDTH)),
    "g_v_sign": ("sign of G's V coefficient", _where(RANDOM + ("table", "flat"))),
}
DEFECTS_OUT = {
    "topleft": ("chroma from the top-left pixel instead of the block sum", _where(RANDOM + ("steps",))),
    "no_round_c": ("block sum floored: + 32768 missing", _where(RANDOM[2:] + ("steps",))),
    "no_oy": ("oy missing", _where(RANDOM + ("flat", "steps"), ranges=(False,))),
    "rb_swap": ("R and B swapped", _where(RANDOM + ("flat", "steps"))),
    "v_at_u": ("V written at U's offset", _where(RANDOM + ("flat", "steps"))),
    "nv21": ("nv12 pairs written V, U", _where(RANDOM + ("flat", "steps"), ("nv12",))),
    "odd_rows_y": ("odd rows of Y dropped", _where(RANDOM + ("flat", "steps"))),
    "no_clip_c": ("chroma clip missing under full_range", _where(("flat",), ranges=(True,))),
    "drop_tail": ("last W % 8 columns dropped", _where(ODD_WIDTH)),
}
