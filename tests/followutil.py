"""Helpers of tests/test_follow_cpu.py, tests/test_follow_gpu.py and tests/test_follow_sensitivity_cpu.py: the CPU
restatement of ``gcv_track_match`` (include/genconvit_hip.h states the arithmetic; this file is written from that statement,
in numpy and Python integers), a second, independent writing of it that can be given a defect, and the synthetic videos and
jobs the GPU test compares on.  No tests here."""
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


# ----------------------------------------------------------------------------- inputs that decide what the others leave open
def largest_case():
    """(frames, jobs) of the largest configuration, grid 64: 3 x 256 x 256 frames, 12 jobs with boxes of 64 ... 120"""
    return fuzz_case(H=256, W=256, n=12, lo=64, hi=120, seed=23)


def tie_case(grid, k):
    """(frames, jobs): two identical frames of 160 x 160 with R = G = B = g[y + x], g seeded noise of length H + W, so luma is
    the value itself and a shift by ``k`` pixels in y reads the same pixels as a shift by ``k`` in x.  Both templates of both
    jobs are one box of side ``grid * k`` (a cell is k x k pixels) at (50, 60) in frame 0.  Job A's prior lies ``k`` pixels
    to the left: every candidate on the anti-diagonal dy + dx = +1 cell costs 0, and only the key's d2, then dy before dx,
    picks (0, +1).  Job B's prior lies ``2 k`` pixels down: cost 0 on dy + dx = -2, where d2 alone picks (-1, -1)."""
    H = W = 160
    g = np.random.default_rng(41).integers(0, 256, H + W, dtype=np.uint8)
    y, x = np.mgrid[0:H, 0:W]
    frames = np.repeat(np.repeat(g[y + x][None, :, :, None], 2, axis=0), 3, axis=3)
    s = grid * k
    tpl = (0, 50, 60 + s, 50 + s, 60)
    jobs = [(1, 50, 60 - k + s, 50 + s, 60 - k, *tpl, 1, *tpl, 1),
            (1, 50 + 2 * k, 60 + s, 50 + 2 * k + s, 60, *tpl, 2, *tpl, 1)]
    return frames, jobs


def far_tie_case(grid, k, up=8, left=7):
    """(frames, jobs): ``tie_case``'s frames and template, one job whose prior lies ``up * k`` pixels up and ``left * k`` to the
    left.  At radius 8 all 289 candidates are valid and those on dy + dx = up + left cost 0.  (8, 7): only (7, 8) and (8, 7),
    candidates 271 and 287, both in the second trip of the 256-lane loop and of equal d2, so dy decides for (7, 8).
    (6, 6): d2 picks (6, 6), candidate 252, which the fourth wave holds."""
    frames, jobs = tie_case(grid, k)
    s = grid * k
    return frames, [(1, 50 - up * k, 60 - left * k + s, 50 - up * k + s, 60 - left * k, *jobs[0][5:])]


TIE_CASES = ((16, 3, 4), (16, 3, 8), (32, 2, 8))            # (grid, k, radius); radius 8: 289 candidates, so equal keys sit
TIE_ROWS = {(16, 3, 4): [[0, 3, 0, 21246], [-3, -3, 0, 28962]],          # in different waves and in the second loop trip
            (16, 3, 8): [[0, 3, 0, 21246], [-3, -3, 0, 28962]],
            (32, 2, 8): [[0, 2, 0, 95744], [-2, -2, 0, 177147]]}
COST_BOUND = 1024 * 64 * 64 * 255                            # 1 069 547 520: what the kernel states as < 2^31


def bound_case():
    """(frames, jobs, grid, radius): the largest cost there is.  Frame 0 black, frame 1 white, 80 x 88; grid 64, both templates
    black boxes, the window white, wa + wb = 1024: every candidate costs 1024 * 4096 * 255 (the one with wa = 1024, wb = 0
    puts all of it through one product), so the key's tie-break answers (0, 0)."""
    frames = np.zeros((2, 80, 88, 3), dtype=np.uint8)
    frames[1] = 255
    a, b = (0, 2, 75, 70, 5), (0, 10, 84, 79, 20)
    jobs = [(1, 6, 82, 72, 12, *a, 1000, *b, 24), (1, 0, 64, 64, 0, *b, 1024, *a, 0), (1, 16, 88, 80, 24, *a, 1, *b, 1023)]
    return frames, jobs, 64, 3


# ----------------------------------------------------------------------------- the same row, written again, with defects
DEFECTS = ("luma without rounding", "cell mean floored", "edges truncated toward zero",
           "validity: top off by one", "validity: bottom off by one", "validity: left off by one",
           "validity: right off by one", "window from template a's frame", "template b built with a's edges",
           "templates swapped", "cost0 equal to the best cost", "oy / ox in cells", "ox scaled by h",
           "tie-break: d2 dropped", "tie-break: dx before dy", "tie-break: the last equal candidate wins",
           "the last candidate is never evaluated", "candidates of the second loop trip dropped",
           "one wave's minimum ignored", "template sums in 16 bits", "the key keeps 29 bits of cost")


def _integral(Y):
    """(H + 1, W + 1) int64: I[y, x] = the sum of Y[:y, :x]"""
    out = np.zeros((Y.shape[0] + 1, Y.shape[1] + 1), dtype=np.int64)
    out[1:, 1:] = Y.cumsum(0).cumsum(1)
    return out


def _cells_alt(I, top, left, ys, xs, floored=False):
    """``_cells`` from an integral image.  Edges outside the frame are clamped to it (only a defect puts them there: a
    kernel with that defect reads other bytes, and what counts here is that the cells differ); an empty cell is 0."""
    ys = np.clip(np.asarray(ys, dtype=np.int64) + top, 0, I.shape[0] - 1)
    xs = np.clip(np.asarray(xs, dtype=np.int64) + left, 0, I.shape[1] - 1)
    y0, y1, x0, x1 = ys[:-1, None], ys[1:, None], xs[None, :-1], xs[None, 1:]
    sums = I[y1, x1] - I[y0, x1] - I[y1, x0] + I[y0, x0]
    cnt = np.maximum((y1 - y0) * (x1 - x0), 1)
    return sums // cnt if floored else (sums + cnt // 2) // cnt


def track_match_alt(frames, jobs, grid, radius, defect=None):
    """``track_match_ref`` written a second time, phase by phase as csrc/follow.hip runs them (edges at index u + R, the valid
    range walked outward from 0, cells from an integral image, the candidates numbered c = cy * nx + cx and dealt over 256
    lanes, the smallest packed key); ``defect``: None, or one of ``DEFECTS``, a way in which such a kernel could plausibly be
    wrong.  Left out, because they cannot change a result: the four validity comparisons off by one in the OTHER direction
    (one candidate too many reads outside the frame, which a restatement cannot follow), and window cells built outside the
    valid candidates' reach (never read)."""
    assert defect is None or defect in DEFECTS, defect
    fr = frames.cpu().numpy() if hasattr(frames, "cpu") else np.asarray(frames)
    f = fr.astype(np.int64)
    Y = (77 * f[..., 0] + 150 * f[..., 1] + 29 * f[..., 2] + (0 if defect == "luma without rounding" else 128)) >> 8
    H, W = Y.shape[1:]
    G, R = int(grid), int(radius)
    integral = {}

    def image(k):
        if k not in integral:
            integral[k] = _integral(Y[k])
        return integral[k]

    def e(u, extent):
        p = int(u) * int(extent)
        return -((-p) // G) if defect == "edges truncated toward zero" and p < 0 else p // G
    floored = defect == "cell mean floored"
    jobs = np.asarray(jobs, dtype=np.int64).reshape(-1, 17)
    out = np.zeros((len(jobs), 4), dtype=np.int32)
    for n, row in enumerate(jobs.tolist()):
        fs, top, right, bottom, left = row[0:5]
        a, wa, b, wb = row[5:10], row[10], row[11:16], row[16]
        h, w = bottom - top, right - left
        ey, ex = [e(u, h) for u in range(-R, G + R + 1)], [e(v, w) for v in range(-R, G + R + 1)]    # index u + R
        off = {k: int(defect == f"validity: {k} off by one") for k in ("top", "bottom", "left", "right")}
        dy_lo = dy_hi = dx_lo = dx_hi = 0
        while dy_lo > -R and top + ey[dy_lo - 1 + R] >= off["top"]:
            dy_lo -= 1
        while dy_hi < R and bottom + ey[dy_hi + 1 + R] <= H - off["bottom"]:
            dy_hi += 1
        while dx_lo > -R and left + ex[dx_lo - 1 + R] >= off["left"]:
            dx_lo -= 1
        while dx_hi < R and right + ex[dx_hi + 1 + R] <= W - off["right"]:
            dx_hi += 1

        def template(box, like):
            hh, ww = like[3] - like[1], like[2] - like[4]
            return _cells_alt(image(box[0]), box[1], box[4], [e(u, hh) for u in range(G + 1)], [e(v, ww) for v in range(G + 1)],
                              floored)
        A, B = template(a, a), template(b, a if defect == "template b built with a's edges" else b)
        if defect == "templates swapped":
            A, B = B, A
        V = _cells_alt(image(a[0] if defect == "window from template a's frame" else fs), top, left,
                       ey[dy_lo + R:dy_hi + G + R + 1], ex[dx_lo + R:dx_hi + G + R + 1], floored)
        ny, nx = dy_hi - dy_lo + 1, dx_hi - dx_lo + 1
        cost = np.zeros((ny, nx), dtype=np.int64)
        for cy in range(ny):                                 # a row of candidates at a time: (nx, G, G)
            win = np.lib.stride_tricks.sliding_window_view(V[cy:cy + G], (G, G))[0]
            sa, sb = np.abs(win - A).sum((-1, -2)), np.abs(win - B).sum((-1, -2))
            if defect == "template sums in 16 bits":
                sa, sb = sa & 0xFFFF, sb & 0xFFFF
            cost[cy] = wa * sa + wb * sb
        best, cost0 = None, 0
        for c in range(ny * nx):
            if (defect == "the last candidate is never evaluated" and c == ny * nx - 1) or \
                    (defect == "candidates of the second loop trip dropped" and c >= 256):
                continue                                     # (cost0 of a candidate that is not evaluated: whatever LDS held; 0)
            cy, cx = divmod(c, nx)
            dy, dx, k = dy_lo + cy, dx_lo + cx, int(cost[cy, cx])
            if dy == 0 and dx == 0:
                cost0 = k
            if defect == "one wave's minimum ignored" and c % 256 >= 192:
                continue                                     # the fourth wave's entry of the cross-wave reduce
            if defect == "the key keeps 29 bits of cost":
                k %= 2 ** 29
            key = (k, dy * dy + dx * dx, dy, dx)
            if defect == "tie-break: d2 dropped":
                key = (k, 0, dy, dx)
            elif defect == "tie-break: dx before dy":
                key = (k, key[1], dx, dy)
            elif defect == "tie-break: the last equal candidate wins":
                key = (k, key[1], -c, 0)
            if best is None or key < best[0]:
                best = (key, k, dy, dx)
        if best is None:
            out[n] = (0, 0, -1, cost0)
            continue
        _, k, dy, dx = best
        oy, ox = e(dy, h), e(dx, w)
        if defect == "oy / ox in cells":
            oy, ox = dy, dx
        elif defect == "ox scaled by h":
            ox = e(dx, h)
        out[n] = (oy, ox, k, k if defect == "cost0 equal to the best cost" else cost0)
    return out
