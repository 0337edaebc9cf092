"""Helpers of tests/test_follow_cpu.py and tests/test_follow_gpu.py: the CPU restatement of ``gcv_track_match``
(include/genconvit_hip.h states the arithmetic; this file is written from that statement, in numpy and Python integers)
and the synthetic videos the tests follow a face through.  No tests here."""
import numpy as np


def edge(u, extent, grid):
    """e(u) = (u * extent) // grid, floor division also for negative u (Python's //)."""
    return (int(u) * int(extent)) // int(grid)


def luma(frames):
    """Y = (77 R + 150 G + 29 B + 128) >> 8 of uint8 (..., 3) pixels, int64."""
    f = np.asarray(frames).astype(np.int64)
    return (77 * f[..., 0] + 150 * f[..., 1] + 29 * f[..., 2] + 128) >> 8


def _cells(Y, top, left, ys, xs):
    """Cell values of one luma frame: rows [top + ys[i], top + ys[i + 1]) x columns [left + xs[k], left + xs[k + 1]),
    (sum + cnt // 2) // cnt.  The edges are strictly increasing (no cell is empty) and inside the frame."""
    ys, xs = np.asarray(ys, dtype=np.int64) + top, np.asarray(xs, dtype=np.int64) + left
    assert ys[0] >= 0 and xs[0] >= 0 and ys[-1] <= Y.shape[0] and xs[-1] <= Y.shape[1]
    assert (np.diff(ys) > 0).all() and (np.diff(xs) > 0).all()
    region = Y[ys[0]:ys[-1], xs[0]:xs[-1]]
    sums = np.add.reduceat(np.add.reduceat(region, ys[:-1] - ys[0], axis=0), xs[:-1] - xs[0], axis=1)
    cnt = np.diff(ys)[:, None] * np.diff(xs)[None, :]
    return (sums + cnt // 2) // cnt


def track_match_ref(frames, jobs, grid, radius):
    """``_lib.track_match`` on the CPU: int32 (n,4) rows (oy, ox, best cost, cost at zero displacement).  ``frames``:
    uint8 (F,H,W,3), numpy or tensor; ``jobs``: (n,17) integers.  The rows must be valid (boxes inside the frame, every
    side >= grid): this is the restatement, not the checks."""
    fr = frames.cpu().numpy() if hasattr(frames, "cpu") else np.asarray(frames)
    Y = luma(fr)
    H, W = Y.shape[1:]
    G, R = int(grid), int(radius)
    jobs = np.asarray(jobs, dtype=np.int64).reshape(-1, 17)
    out = np.zeros((len(jobs), 4), dtype=np.int32)
    for n, row in enumerate(jobs):
        fs, top, right, bottom, left = (int(v) for v in row[0:5])
        h, w = bottom - top, right - left
        tpl = []
        for c in (5, 11):
            f, t, r, b, l = (int(v) for v in row[c:c + 5])
            assert b - t >= G and r - l >= G
            tpl.append(_cells(Y[f], t, l, [edge(u, b - t, G) for u in range(G + 1)], [edge(v, r - l, G) for v in range(G + 1)]))
        A, B = tpl
        wa, wb = int(row[10]), int(row[16])
        assert h >= G and w >= G and wa >= 0 and wb >= 0 and 1 <= wa + wb <= 1024
        # valid displacements, and the window cells they use: everything else is never read
        dys = [d for d in range(-R, R + 1) if 0 <= top + edge(d, h, G) and top + edge(d, h, G) + h <= H]
        dxs = [d for d in range(-R, R + 1) if 0 <= left + edge(d, w, G) and left + edge(d, w, G) + w <= W]
        assert 0 in dys and 0 in dxs and dys == list(range(dys[0], dys[-1] + 1)) and dxs == list(range(dxs[0], dxs[-1] + 1))
        V = _cells(Y[fs], top, left, [edge(u, h, G) for u in range(dys[0], dys[-1] + G + 1)],
                   [edge(v, w, G) for v in range(dxs[0], dxs[-1] + G + 1)])          # V[u - dys[0]][v - dxs[0]]
        best = None
        for dy in dys:
            for dx in dxs:
                win = V[dy - dys[0]:dy - dys[0] + G, dx - dxs[0]:dx - dxs[0] + G]
                cost = int(wa * np.abs(A - win).sum() + wb * np.abs(B - win).sum())
                key = (cost, dy * dy + dx * dx, dy, dx)
                if best is None or key < best:
                    best = key
                if dy == 0 and dx == 0:
                    cost0 = cost
        out[n] = (edge(best[2], h, G), edge(best[3], w, G), best[0], cost0)
    return out


# ----------------------------------------------------------------------------- synthetic videos
PATH_TOPLEFT = [(20, 30), (29, 35), (32, 40), (33, 50), (32, 60)]          # (top, left) of the 48 x 40 patch in frames 0 .. 4
PATH_H, PATH_W = 48, 40


def background(nf, H, W):
    """((2y + x + 7f) % 256, (3x + f) % 256, (y + 2x) % 256): smooth, and it drifts from frame to frame."""
    f, y, x = np.meshgrid(np.arange(nf), np.arange(H), np.arange(W), indexing="ij")
    return np.stack([(2 * y + x + 7 * f) % 256, (3 * x + f) % 256, (y + 2 * x) % 256], -1).astype(np.uint8)


def path_case():
    """(frames, jobs, priors): 5 frames of 96 x 128, a 48 x 40 patch of noise on the path above over the drifting
    background; the detector saw frames 0 and 4, the three frames between are to be followed from the interpolated priors
    with weights (4 - k, k)."""
    frames = background(5, 96, 128)
    patch = np.random.default_rng(3).integers(0, 256, (PATH_H, PATH_W, 3), dtype=np.uint8)
    for f, (t, l) in enumerate(PATH_TOPLEFT):
        frames[f, t:t + PATH_H, l:l + PATH_W] = patch
    box = lambda f, t, l: (f, t, l + PATH_W, t + PATH_H, l)
    a, b = box(0, *PATH_TOPLEFT[0]), box(4, *PATH_TOPLEFT[4])
    priors = [(23, 38), (26, 45), (29, 53)]                  # floor(a + (b - a) k / 4 + 0.5) per coordinate
    jobs = [(*box(k, *priors[k - 1]), *a, 4 - k, *b, k) for k in (1, 2, 3)]
    return frames, jobs, priors


PATH_FOLLOWED = [(29, 35), (32, 40), (32, 50)]               # the third is one pixel off the truth: a cell is 3 pixels high


def two_face_video():
    """(frames, detections): 9 frames of 96 x 128 made like the path case — the noise patch moves on a curve, seen by the
    detector on frames 0, 4 and 8 — plus a second, static 40 x 24 face of noise at the left border that the patch never
    covers.  ``detections``: rows (frame, top, right, bottom, left) of both faces on frames 0, 4, 8."""
    path = PATH_TOPLEFT + [(29, 66), (25, 72), (20, 80), (14, 86)]
    frames = background(9, 96, 128)
    rng = np.random.default_rng(3)
    patch = rng.integers(0, 256, (PATH_H, PATH_W, 3), dtype=np.uint8)
    still = rng.integers(0, 256, (40, 24, 3), dtype=np.uint8)
    for f, (t, l) in enumerate(path):
        frames[f, t:t + PATH_H, l:l + PATH_W] = patch
        frames[f, 50:90, 2:26] = still
    det = []
    for f in (0, 4, 8):
        t, l = path[f]
        det += [(f, t, l + PATH_W, t + PATH_H, l), (f, 50, 26, 90, 2)]
    return frames, det, path


def fuzz_case(nf=3, H=120, W=160, n=48, lo=16, hi=100, seed=17, smooth=True):
    """(frames, jobs): ``nf`` frames of H x W — noise, the last one smooth ((3y + x) % 256 etc.: cost ties) — and ``n``
    random jobs: box sides lo .. hi that are no multiple of 16, the three boxes of a job of three different sizes, weights
    that include wa = 0 and wb = 0 (the other positive), and priors that touch each of the four borders."""
    rng = np.random.default_rng(seed)
    frames = rng.integers(0, 256, (nf, H, W, 3), dtype=np.uint8)
    if smooth:
        y, x = np.mgrid[0:H, 0:W]
        frames[nf - 1] = np.stack([(3 * y + x) % 256, (2 * x + y) % 256, (y * x // 7) % 256], -1).astype(np.uint8)
    hi_h, hi_w = min(hi, H), min(hi, W)

    def side(top, taken=()):
        while True:
            s = int(rng.integers(lo, top + 1))
            if (s % 16 or lo == top) and s not in taken:
                return s

    def box(h, w, where=None):
        top, left = int(rng.integers(0, H - h + 1)), int(rng.integers(0, W - w + 1))
        top = {"top": 0, "bottom": H - h}.get(where, top)
        left = {"left": 0, "right": W - w}.get(where, left)
        return (int(rng.integers(0, nf)), top, left + w, top + h, left)
    jobs = []
    for i in range(n):
        hs, wsd = [], []
        for _ in range(3):
            hs.append(side(hi_h, hs))
            wsd.append(side(hi_w, wsd))
        where = ("top", "bottom", "left", "right")[i % 8] if i % 8 < 4 else None
        wa, wb = [(0, 5), (7, 0), (1, 1), (1023, 1)][i % 4] if i % 3 == 0 else (int(rng.integers(0, 9)), int(rng.integers(1, 9)))
        jobs.append((*box(hs[0], wsd[0], where), *box(hs[1], wsd[1]), wa, *box(hs[2], wsd[2]), wb))
    return frames, jobs
