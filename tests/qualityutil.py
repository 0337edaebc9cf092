"""Helpers of tests/test_quality_cpu.py, tests/test_quality_gpu.py and tests/test_quality_sensitivity_cpu.py: the CPU
restatement of ``gcv_face_quality`` (include/genconvit_hip.h states the arithmetic; this file is written from that
statement, in numpy int64), a second writing of it that can be given a defect, and the synthetic material the tests
measure: a noise texture, box blurs, flat patches, the boxes of the GPU test, a checkerboard at the largest sums, and a small
two-face video with a blurred run.  No tests here."""
import numpy as np

from tests import followutil as fu


def cells_ref(Y, box, grid):
    """The (G, G) int64 cell values of ``box`` = (top, right, bottom, left) in the luma frame ``Y``, and the row and column
    edges relative to the box: cell (u, v) is (sum of Y + cnt // 2) // cnt over rows [ey[u], ey[u + 1]) x columns
    [ex[v], ex[v + 1]) with e(u) = (u extent) // G."""
    top, right, bottom, left = (int(v) for v in box)
    G, h, w = int(grid), bottom - top, right - left
    assert h >= G and w >= G and 0 <= top and 0 <= left and bottom <= Y.shape[0] and right <= Y.shape[1]
    ey = np.array([fu.edge(u, h, G) for u in range(G + 1)], dtype=np.int64)
    ex = np.array([fu.edge(v, w, G) for v in range(G + 1)], dtype=np.int64)
    region = np.asarray(Y, dtype=np.int64)[top:bottom, left:right]
    sums = np.add.reduceat(np.add.reduceat(region, ey[:-1], axis=0), ex[:-1], axis=1)
    cnt = np.diff(ey)[:, None] * np.diff(ex)[None, :]
    return (sums + cnt // 2) // cnt, ey, ex


def quality_of_cells(c):
    """The row (G, S1, S2, L2, GX, GY, dark, bright) of a (G, G) array of cell values, int64."""
    c = np.asarray(c, dtype=np.int64)
    G = c.shape[0]
    lap = 4 * c[1:-1, 1:-1] - c[:-2, 1:-1] - c[2:, 1:-1] - c[1:-1, :-2] - c[1:-1, 2:]
    dx, dy = c[:, 1:] - c[:, :-1], c[1:, :] - c[:-1, :]
    return np.array([G, c.sum(), (c * c).sum(), (lap * lap).sum(), (dx * dx).sum(), (dy * dy).sum(), (c < 16).sum(),
                     (c > 239).sum()], dtype=np.int64)


def face_quality_ref(frames, boxes, grid):
    """``_lib.face_quality`` on the CPU: int64 (n,8) rows (G, S1, S2, L2, GX, GY, dark, bright).  ``frames``: uint8
    (F,H,W,3), numpy or tensor; ``boxes``: (n,5) integers.  The rows must be valid (inside the frame, every side >= grid):
    this is the restatement, not the checks."""
    fr = frames.cpu().numpy() if hasattr(frames, "cpu") else np.asarray(frames)
    boxes = np.asarray(boxes, dtype=np.int64).reshape(-1, 5)
    out = np.zeros((len(boxes), 8), dtype=np.int64)
    luma = {}
    for n, (f, *box) in enumerate(boxes.tolist()):
        if f not in luma:
            luma[f] = fu.luma(fr[f])
        out[n] = quality_of_cells(cells_ref(luma[f], box, grid)[0])
    return out


def measures(raw):
    """sharpness, gx, gy of (n,8) rows as ``pred_func.face_quality`` defines them, float64"""
    raw = np.asarray(raw, dtype=np.int64).reshape(-1, 8)
    g = raw[:, 0].astype(np.float64)
    return raw[:, 3] / ((g - 2) * (g - 2)), raw[:, 4] / (g * (g - 1)), raw[:, 5] / (g * (g - 1))


# ----------------------------------------------------------------------------- synthetic material
def texture(h, w, feature=4, seed=1):
    """uint8 (h, w, 3) grey noise whose features are ``feature`` x ``feature`` pixel blocks (R = G = B, so Y = the value)"""
    rng = np.random.default_rng(seed)
    small = rng.integers(0, 256, (-(-h // feature), -(-w // feature)), dtype=np.uint8)
    img = np.repeat(np.repeat(small, feature, axis=0), feature, axis=1)[:h, :w]
    return np.repeat(img[:, :, None], 3, axis=2)


def box_blur(img, ky=1, kx=1):
    """The mean over a ``ky`` x ``kx`` window (odd sizes) around every pixel, edges replicated, rounded to nearest: uint8
    of the same shape.  ``ky`` = 1 blurs along the rows only (a horizontal motion blur)."""
    assert ky % 2 == 1 and kx % 2 == 1
    out = np.asarray(img).astype(np.int64)
    for axis, k in ((0, ky), (1, kx)):
        if k > 1:
            pad = [(0, 0)] * out.ndim
            pad[axis] = (k // 2 + 1, k // 2)
            cs = np.cumsum(np.pad(out, pad, mode="edge"), axis=axis)
            n = out.shape[axis]
            s = np.take(cs, np.arange(k, k + n), axis=axis) - np.take(cs, np.arange(0, n), axis=axis)
            out = (s + k // 2) // k
    return out.astype(np.uint8)


def flat(h, w, value):
    """uint8 (h, w, 3) of one value: ``flat(h, w, 0)`` is black, ``flat(h, w, 255)`` white"""
    return np.full((h, w, 3), value, dtype=np.uint8)


FACE_A, FACE_B = (20, 70, 68, 30), (50, 120, 90, 80)         # (top, right, bottom, left): 48 x 40 and 40 x 40 pixels
PLANTED = (4, 5, 6)                                          # the frames in which face A is blurred


def gated_video(black_b=False):
    """(frames, detections): 10 frames of 96 x 128 over followutil's drifting background with two static faces of noise
    texture; face A is box-blurred by 9 pixels in the frames ``PLANTED``; ``black_b`` paints face B black in every frame.
    ``detections``: rows (frame, top, right, bottom, left), face A then face B, frame by frame."""
    frames = fu.background(10, 96, 128)
    a = texture(FACE_A[2] - FACE_A[0], FACE_A[1] - FACE_A[3], seed=2)
    b = texture(FACE_B[2] - FACE_B[0], FACE_B[1] - FACE_B[3], seed=3)
    soft = box_blur(a, 9, 9)
    det = []
    for f in range(10):
        frames[f, FACE_A[0]:FACE_A[2], FACE_A[3]:FACE_A[1]] = soft if f in PLANTED else a
        frames[f, FACE_B[0]:FACE_B[2], FACE_B[3]:FACE_B[1]] = 0 if black_b else b
        det += [(f, *FACE_A), (f, *FACE_B)]
    return frames, det


# ----------------------------------------------------------------------------- the inputs of the GPU test
def corners(f, H, W, h, w):
    """a box of h x w in each corner of frame ``f``"""
    return [(f, 0, w, h, 0), (f, 0, W, h, W - w), (f, H - h, w, H, 0), (f, H - h, W, H, W - w)]


def fuzz_boxes(grid):
    """(frames, boxes): followutil's 3 x 120 x 160 frames (two of noise, a smooth one) and the 48 prior boxes of its jobs:
    sides from the grid to 100 that are no multiple of 16, touching each of the four borders"""
    frames, jobs = fu.fuzz_case(lo=grid)
    return frames, [tuple(j[:5]) for j in jobs]


def edge_boxes(grid):
    """boxes on the 120 x 160 frames of ``fuzz_boxes``: one pixel over the grid in one direction, exactly the grid, the whole
    frame, and a box in each corner of the frame"""
    boxes = [(0, 7, 11 + grid + 1, 7 + grid, 11), (1, 7, 11 + grid, 7 + grid + 1, 11), (2, 3, 5 + grid, 3 + grid, 5),
             (0, 0, 160, 120, 0), (2, 0, 160, 120, 0)]
    return boxes + corners(1, 120, 160, grid + 5, grid + 21) + corners(2, 120, 160, 67, 71)


def flat_case():
    """(frames, boxes): 3 x 70 x 90, flat Y = 124, black and white; the whole frame and a box inside it"""
    frames = np.stack([flat(70, 90, 0), flat(70, 90, 0), flat(70, 90, 255)])
    frames[0] = (10, 200, 30)                                                              # Y = 124
    return frames, [(f, 0, 90, 70, 0) for f in range(3)] + [(f, 2, 88, 69, 1) for f in range(3)]


def unaligned_case():
    """(frames, boxes): 4 x 37 x 53 noise, of which the test takes frames[1:] (5 883 bytes into the allocation), and boxes
    on those three frames"""
    frames = np.random.default_rng(31).integers(0, 256, (4, 37, 53, 3), dtype=np.uint8)
    boxes = [(f, 0, 53, 37, 0) for f in range(3)] + corners(0, 37, 53, 16, 17) + corners(2, 37, 53, 21, 16) + \
        [(1, 9, 40, 30, 12)]
    return frames, boxes


def largest_case():
    """(frames, boxes): 2 frames of 300 x 400, noise and a blurred texture, with the whole frame as a box"""
    frames = np.random.default_rng(32).integers(0, 256, (2, 300, 400, 3), dtype=np.uint8)
    frames[1] = box_blur(texture(300, 400, seed=6), 3, 3)
    return frames, [(0, 0, 400, 300, 0), (1, 0, 400, 300, 0), (1, 13, 399, 300, 101), (0, 100, 164, 164, 100)]


def checkerboard(grid, k):
    """(frames, boxes): one frame of ``grid * k`` pixels a side, squares of ``k`` x ``k`` pixels that alternate between 0 and
    255, and the whole frame as the box: the cells are the squares, every interior Laplacian is +-1020 and every difference
    +-255.  At grid 64 L2 = 62^2 * 1020^2 = 3 999 297 600, more than 2^31, and a lane's 16 cells reach 16 * 1020^2."""
    side = grid * k
    y, x = np.mgrid[0:side, 0:side]
    img = (((y // k + x // k) % 2) * 255).astype(np.uint8)
    return np.repeat(img[None, :, :, None], 3, axis=3), [(0, 0, side, side, 0)]


CHECKERBOARD_64 = [64, 522240, 133171200, 3999297600, 262180800, 262180800, 2048, 2048]


# ----------------------------------------------------------------------------- the same rows, written again, with defects
DEFECTS = ("luma without rounding", "cell mean floored", "row edges from w, column edges from h", "dark <= 16",
           "bright >= 239", "GX wraps at the last column", "GY wraps at the last row",
           "the Laplacian over border cells, neighbours clamped", "GX / GY swapped",
           "cells of the later 256-cell trips dropped", "one wave's partial dropped", "totals in signed 32 bits",
           "S2 in 24 bits")


def face_quality_alt(frames, boxes, grid, defect=None):
    """``face_quality_ref`` written a second time, the way csrc/quality.hip runs: the cells from an integral image as one flat
    list, cell i the work of thread i % 256 (wave (i % 256) // 64) in trip i // 256, every term per cell with its neighbours
    by index, and the seven sums over the cells.  ``defect``: None or one of ``DEFECTS``.  "GX wraps": the right neighbour
    is cell i + 1 also at the last column (the next row's first cell; the last cell of all has none and adds 0, where a
    kernel would read behind the cells); "GY wraps": the lower neighbour of the last row is the first row."""
    assert defect is None or defect in DEFECTS, defect
    fr = frames.cpu().numpy() if hasattr(frames, "cpu") else np.asarray(frames)
    f = fr.astype(np.int64)
    Y = (77 * f[..., 0] + 150 * f[..., 1] + 29 * f[..., 2] + (0 if defect == "luma without rounding" else 128)) >> 8
    G = int(grid)
    GG = G * G
    i = np.arange(GG)
    u, v = i // G, i % G
    integral = {}
    out = np.zeros((len(boxes), 8), dtype=np.int64)
    for n, (k, top, right, bottom, left) in enumerate(np.asarray(boxes, dtype=np.int64).reshape(-1, 5).tolist()):
        if k not in integral:
            integral[k] = fu._integral(Y[k])
        h, w = bottom - top, right - left
        if defect == "row edges from w, column edges from h":
            h, w = w, h
        c = fu._cells_alt(integral[k], top, left, [(a * h) // G for a in range(G + 1)], [(a * w) // G for a in range(G + 1)],
                          floored=defect == "cell mean floored").ravel()
        cr = np.where(v < G - 1, c[np.minimum(i + 1, GG - 1)], c)
        cb = np.where(u < G - 1, c[np.minimum(i + G, GG - 1)], c)
        if defect == "GX wraps at the last column":
            cr = c[np.minimum(i + 1, GG - 1)]
        if defect == "GY wraps at the last row":
            cb = c[(i + G) % GG]
        inner = (u >= 1) & (u < G - 1) & (v >= 1) & (v < G - 1)
        if defect == "the Laplacian over border cells, neighbours clamped":
            up, lf = np.where(u >= 1, c[np.maximum(i - G, 0)], c), np.where(v >= 1, c[np.maximum(i - 1, 0)], c)
            lap = 4 * c - up - cb - lf - cr
        else:
            lap = np.where(inner, 4 * c - c[np.maximum(i - G, 0)] - cb - c[np.maximum(i - 1, 0)] - cr, 0)
        gx, gy = (cr - c) ** 2, (cb - c) ** 2
        if defect == "GX / GY swapped":
            gx, gy = gy, gx
        terms = [c, c * c, lap * lap, gx, gy, c <= 16 if defect == "dark <= 16" else c < 16,
                 c >= 239 if defect == "bright >= 239" else c > 239]
        keep = np.ones(GG, dtype=bool)
        if defect == "cells of the later 256-cell trips dropped":
            keep = i < 256
        if defect == "one wave's partial dropped":
            keep = i % 256 < 192
        sums = [int(np.asarray(t, dtype=np.int64)[keep].sum()) for t in terms]
        if defect == "totals in signed 32 bits":
            sums = [(s + 2 ** 31) % 2 ** 32 - 2 ** 31 for s in sums]
        if defect == "S2 in 24 bits":
            sums[1] %= 2 ** 24
        out[n] = [G] + sums
    return out
