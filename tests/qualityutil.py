"""Helpers of tests/test_quality_cpu.py and tests/test_quality_gpu.py: the CPU restatement of ``gcv_face_quality``
(include/genconvit_hip.h states the arithmetic; this file is written from that statement, in numpy int64) and the synthetic
material the tests measure: a noise texture, box blurs, flat patches, and a small two-face video with a blurred run.  No
tests here."""
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
