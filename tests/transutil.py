"""Helpers of tests/test_transitions_cpu.py, tests/test_transitions_gpu.py and tests/test_transitions_sensitivity_cpu.py: the
CPU restatement of ``gcv_frame_cells``, ``gcv_blend_fit`` and ``gcv_hist_diff_lag`` (include/genconvit_hip.h states the
arithmetic; this file is written from that statement: cells by slices, fits in Python integers), of the rule
``pred_func.shot_transitions`` applies to them, a second writing of the first two that can be given a defect (the third's
is ``cutsutil.hist_diff_alt``), and the synthetic videos.  No tests here."""
import numpy as np
import torch

from tests import cutsutil as cu

DEFAULTS = dict(lags=(4, 8), grid=16, regions=4, h_min=0.25, rho_max=0.05, a_lo=0.1, a_hi=0.9, slack=0.05)


def _numpy(x):
    return x.cpu().numpy() if hasattr(x, "cpu") else np.asarray(x)


# ----------------------------------------------------------------------------- the three device entries, restated
def frame_cells_ref(frames, grid):
    """``_lib.frame_cells`` on the CPU: int64 (F, grid^2), cell u * grid + v = the sum of Y over rows [(u H) // G,
    ((u + 1) H) // G) and the columns alike."""
    y = cu.luma(_numpy(frames))
    F, H, W = y.shape
    ey, ex = cu.edges(H, grid), cu.edges(W, grid)
    out = np.zeros((F, grid * grid), dtype=np.int64)
    for u in range(grid):
        for v in range(grid):
            out[:, u * grid + v] = y[:, ey[u]:ey[u + 1], ex[v]:ex[v + 1]].sum((1, 2))
    return out


def blend_fit_ref(cells, lag):
    """``_lib.blend_fit`` on the CPU in Python integers: int64 (F - lag, 2 lag - 1), rows [Sdd, Smd_1 ..., Smm_1 ...];
    every value is asserted to fit."""
    rows = [[int(v) for v in r] for r in _numpy(cells).tolist()]
    out = []
    for p in range(max(0, len(rows) - lag)):
        a = rows[p]
        d = [y - x for x, y in zip(a, rows[p + lag])]
        ms = [[y - x for x, y in zip(a, rows[p + k])] for k in range(1, lag)]
        row = [sum(v * v for v in d)] + [sum(m * v for m, v in zip(mk, d)) for mk in ms] + [sum(m * m for m in mk) for mk in ms]
        assert all(-2 ** 63 <= v < 2 ** 63 for v in row)
        out.append(row)
    return np.array(out, dtype=np.int64).reshape(len(out), 2 * lag - 1)


def hist_diff_lag_ref(hist, lag):
    """``_lib.hist_diff_lag`` on the CPU: int64 (F - lag, regions^2)"""
    h = _numpy(hist).astype(np.int64)
    return np.abs(h[lag:] - h[:-lag]).sum(-1) if h.shape[0] > lag else np.zeros((0, h.shape[1]), dtype=np.int64)


# ----------------------------------------------------------------------------- the rule
def fit_terms(row, lag):
    """(a_1 ..., rho_1 ...) of one row of the fit, Python floats (float64): the integers are converted before anything
    is multiplied; Sdd == 0 gives a = 0 and rho = inf"""
    sdd = float(int(row[0]))
    if sdd <= 0.0:
        return [0.0] * (lag - 1), [float("inf")] * (lag - 1)
    smd = [float(int(v)) for v in row[1:lag]]
    smm = [float(int(v)) for v in row[lag:]]
    return [v / sdd for v in smd], [(mm - md * md / sdd) / sdd for md, mm in zip(smd, smm)]


def transitions_ref(frames, lags=(4, 8), grid=16, regions=4, h_min=0.25, rho_max=0.05, a_lo=0.1, a_hi=0.9, slack=0.05):
    """``pred_func.shot_transitions`` from the restated entries alone: (transitions, info)"""
    fr = _numpy(frames)
    F, H, W = fr.shape[:3]
    cells, hist = frame_cells_ref(fr, grid), cu.frame_hist_ref(fr, regions)
    marked, info = set(), {}
    for lag in lags:
        fit = blend_fit_ref(cells, lag)
        scores = cu.scores_ref(hist_diff_lag_ref(hist, lag), H, W, regions) if F > lag else np.zeros((0,))
        a = np.zeros((len(fit), lag - 1))
        rho = np.zeros((len(fit), lag - 1))
        blend = np.zeros((len(fit),), dtype=bool)
        for p, row in enumerate(fit):
            ak, rk = fit_terms(row, lag)
            a[p], rho[p] = ak, rk
            inside = [a_lo <= v <= a_hi for v in ak]
            blend[p] = (int(row[0]) > 0 and scores[p] >= h_min and max(rk) <= rho_max and
                        all(y >= x - slack for x, y in zip(ak, ak[1:])) and sum(inside) >= 2)
            if blend[p]:
                marked |= {p + 1 + k for k, m in enumerate(inside) if m}
        info[lag] = {"scores": scores, "a": a, "rho": rho, "blend": blend}
    return runs(marked), info


def runs(marked):
    """the maximal runs of consecutive integers of a set: [(first, last), ...]"""
    out = []
    for f in sorted(marked):
        if out and out[-1][1] == f - 1:
            out[-1] = (out[-1][0], f)
        else:
            out.append((f, f))
    return out


def same_info(got, want):
    """both infos hold the same lags and bit-equal arrays"""
    if sorted(got) != sorted(want):
        return False
    return all(sorted(got[lag]) == sorted(want[lag]) and
               all(np.asarray(got[lag][k]).dtype == np.asarray(want[lag][k]).dtype and
                   np.array_equal(got[lag][k], want[lag][k]) for k in want[lag]) for lag in want)


# ----------------------------------------------------------------------------- the device entries on the CPU
def frame_cells_cpu(frames_u8, grid=16, out=None):
    """stands in for ``_lib.frame_cells`` where there is no GPU: host tensors in, host tensors out"""
    cells = torch.as_tensor(frame_cells_ref(frames_u8, grid).astype(np.int32))
    if out is None:
        return cells
    out.copy_(cells)
    return out


def blend_fit_cpu(cells, lag):
    return torch.as_tensor(blend_fit_ref(cells, lag))


def hist_diff_lag_cpu(hist, lag):
    return torch.as_tensor(hist_diff_lag_ref(hist, lag).astype(np.int32))


# ----------------------------------------------------------------------------- videos
TRANSITIONS = [(8, 13), (30, 34)]
HARD_CUT = 22


def _looks(H=90, W=130):
    """the three looks of ``cutsutil.three_shot_video``"""
    y, x = np.mgrid[0:H, 0:W]
    zero = np.zeros((H, W))
    return [
        np.stack((50 + 40 * x / W, 70 + 30 * x / W, 90 + zero), -1),
        np.stack((90 + 50 * y / H, 100 + 60 * y / H, 80 + 40 * y / H), -1),
        np.where((((y // 13) + (x // 13)) % 2 == 0)[..., None], np.array([60.0, 110.0, 70.0]), np.array([170.0, 150.0, 200.0])),
    ]


def transition_video(seed=7):
    """38 x 90 x 130: frames 0-7 look 0, 8-13 a linear dissolve (a = k / 7) from frame 7's clean picture to frame 14's,
    14-21 look 1, a hard cut, 22-29 look 2, 30-34 frame 29's clean picture fading to black (factor 1 - k / 6), 35-37 black.
    Inside a shot the 36 x 30 skin patch moves by (3, 5) pixels a frame from (6, 10), (40, 60), (20, 40).  Fresh +-6 noise
    per channel is added after the blending, then the frames are clipped."""
    rng = np.random.default_rng(seed)
    looks = _looks()

    def clean(look, py, px, k):
        fr = looks[look].copy()
        fr[py + 3 * k:py + 3 * k + 36, px + 5 * k:px + 5 * k + 30] = cu.SKIN
        return fr
    pics = [clean(0, 6, 10, k) for k in range(8)]
    first = clean(1, 40, 60, 0)
    pics += [(1 - k / 7) * pics[7] + (k / 7) * first for k in range(1, 7)]
    pics += [clean(1, 40, 60, k) for k in range(8)]
    pics += [clean(2, 20, 40, k) for k in range(8)]
    pics += [(1 - k / 6) * pics[29] for k in range(1, 6)]
    pics += [np.zeros_like(pics[0])] * 3
    frames = [np.clip(p + rng.integers(-6, 7, size=p.shape), 0, 255).astype(np.uint8) for p in pics]
    return np.stack(frames)


def pan_video(step, seed=9, F=24, H=90, W=130):
    """a window that slides ``step`` pixels a frame to the right over a random texture of 6-pixel blocks, with fresh +-6
    noise per channel on every frame"""
    rng = np.random.default_rng(seed)
    blocks = rng.integers(30, 226, size=((H + 5) // 6, (W + step * F + 5) // 6, 3))
    wide = np.repeat(np.repeat(blocks, 6, 0), 6, 1).astype(np.float64)
    frames = [np.clip(wide[:H, step * f:step * f + W] + rng.integers(-6, 7, size=(H, W, 3)), 0, 255).astype(np.uint8)
              for f in range(F)]
    return np.stack(frames)


def extreme_cells(grid=8, F=6):
    """(F, grid^2) int32 rows that alternate between 0 and V, the phase flipping from row to row; V is the largest value with
    (grid^2 / 2) V^2 < 2^62, the bound ``gcv_blend_fit`` states for a row (sum of squares < 2^62).  Sdd = grid^2 V^2 is then
    just below 2^63, far beyond what a float64 accumulation holds exactly."""
    import math
    half = grid * grid // 2
    v = math.isqrt((2 ** 62 - 1) // half)
    assert half * v * v < 2 ** 62 <= half * (v + 1) * (v + 1) and v < 2 ** 31
    cells = np.zeros((F, grid * grid), dtype=np.int64)
    for f in range(F):
        cells[f, (f % 2)::2] = v
    cells[2, 0::4] = v // 3                                 # middles off the line, so that Smd and Smm differ
    cells[3, 1::4] = v - 1
    assert all(sum(int(c) ** 2 for c in row) < 2 ** 62 for row in cells)
    return cells.astype(np.int32)


def tiny_video():
    """2 x 32 x 32 noise: at G = 32 a cell is one pixel"""
    return cu.noise_video(F=2, H=32, W=32, seed=13)


def wide_video():
    """1 x 37 x 1103 noise: 276 groups a row, more than the 256 threads"""
    return cu.noise_video(F=1, H=37, W=1103, seed=14)


def flat_video():
    """1 x 512 x 512 flat 255: at G = 8 every cell is 255 * 4096, in 8 slices of 8 pixel rows"""
    return np.full((1, 512, 512, 3), 255, dtype=np.uint8)


def tall_video():
    """2 x 161 x 53 noise: at G = 8 a row of cells has 20-21 pixel rows, in 2 slices of 10 and 10-11"""
    return cu.noise_video(F=2, H=161, W=53, seed=15)


def cells_slices(nframes, H, grid):
    """S of ``launch_frame_cells``: the row slices a row of cells is split into"""
    return cu.launch_slices(nframes * grid, H // grid)


# ----------------------------------------------------------------------------- the same entries, written again, with defects
CELL_DEFECTS = ("luma without rounding", "a group's whole sum given to its first pixel's cell",
                "at most one edge crossed per group", "the cell index taken from x G / W", "column edges rounded",
                "cells transposed", "the slice-boundary row counted twice", "the slice-boundary row dropped")
FIT_DEFECTS = ("D taken at lag - 1", "m relative to B", "the Smd / Smm columns shifted by one k",
               "cells j >= 1 of a thread dropped", "one wave's partial dropped", "products accumulated in float64",
               "products in 32 bits")


def _column_cells(W, G, defect):
    """the cell column every pixel column's luma goes to, as the kernel's 4-pixel groups walk a row: the cell of the group's
    first pixel from one division, then on to the next cell at every edge crossed"""
    half = G // 2 if defect == "column edges rounded" else 0
    ex = [(v * W + half) // G for v in range(G + 1)]
    out = np.zeros(W, dtype=np.int64)
    for x in range(0, W, 4):
        v = (x * G) // W if defect == "the cell index taken from x G / W" else ((x + 1) * G - 1) // W
        while half and not ex[v] <= x < ex[v + 1]:           # rounded edges: the first pixel's cell among those edges
            v += 1 if x >= ex[v + 1] else -1
        first, crossed = v, 0
        for k in range(min(4, W - x)):
            if x + k >= ex[v + 1] and (k or defect != "the cell index taken from x G / W") and \
                    not (defect == "at most one edge crossed per group" and crossed):
                v, crossed = v + 1, crossed + 1
            out[x + k] = first if defect == "a group's whole sum given to its first pixel's cell" else v
    return out


def frame_cells_alt(frames, grid, defect=None):
    """``frame_cells_ref`` written a second time, the way csrc/cuts.hip walks a frame: a map from every pixel to the cell
    that receives its luma (columns by 4-pixel group, rows by row of cells and slice) and one weighted bincount per frame.
    ``defect``: None or one of ``CELL_DEFECTS``.  "the cell index taken from x G / W" is a kernel that trusts x G / W for the
    group's first pixel (it can be one cell short) and looks for edges from the second pixel on."""
    assert defect is None or defect in CELL_DEFECTS, defect
    f = _numpy(frames).astype(np.int64)
    y = (77 * f[..., 0] + 150 * f[..., 1] + 29 * f[..., 2] + (0 if defect == "luma without rounding" else 128)) >> 8
    F, H, W = y.shape
    G = int(grid)
    ey = cu.edges(H, G)
    S = cells_slices(F, H, G)
    col = _column_cells(W, G, defect)
    row, mult = np.zeros(H, dtype=np.int64), np.zeros(H, dtype=np.int64)
    for u in range(G):
        row[ey[u]:ey[u + 1]] = u
        mult[ey[u]:ey[u + 1]] = cu.slice_rows(ey[u], ey[u + 1], S, {"the slice-boundary row counted twice": "twice",
                                                                   "the slice-boundary row dropped": "dropped"}.get(defect))
    cell = col[None, :] * G + row[:, None] if defect == "cells transposed" else row[:, None] * G + col[None, :]
    out = np.zeros((F, G * G), dtype=np.int64)
    for k in range(F):
        out[k] = np.bincount(cell.ravel(), weights=(y[k] * mult[:, None]).ravel(), minlength=G * G).astype(np.int64)
    return out


def blend_fit_alt(cells, lag, defect=None):
    """``blend_fit_ref`` written a second time, in numpy int64 as the kernel's registers hold it (cell c belongs to thread
    c % 256 as its cell c // 256, threads 64 w ... 64 w + 63 are wave w).  ``defect``: None or one of ``FIT_DEFECTS``."""
    assert defect is None or defect in FIT_DEFECTS, defect
    c = _numpy(cells).astype(np.int64)
    F, GG = c.shape
    keep = np.ones(GG, dtype=bool)
    if defect == "cells j >= 1 of a thread dropped":
        keep[256:] = False
    if defect == "one wave's partial dropped" and GG >= 256:
        keep[np.arange(GG) % 256 >= 192] = False

    def dot(p, q):
        prod = p[keep] * q[keep]
        if defect == "products in 32 bits":
            prod = prod.astype(np.int32).astype(np.int64)
        if defect == "products accumulated in float64":
            return int(prod.astype(np.float64).sum())
        return int(prod.sum())
    out = np.zeros((max(0, F - lag), 2 * lag - 1), dtype=np.int64)
    for p in range(max(0, F - lag)):
        a, b = c[p], c[p + lag]
        d = (c[p + lag - 1] if defect == "D taken at lag - 1" else b) - a
        out[p, 0] = dot(d, d)
        for k in range(1, lag):
            m = c[p + (k - 1 if defect == "the Smd / Smm columns shifted by one k" else k)] - \
                (b if defect == "m relative to B" else a)
            out[p, k], out[p, lag - 1 + k] = dot(m, d), dot(m, m)
    return out
