"""Helpers of tests/test_extend_cpu.py, tests/test_extend_gpu.py and tests/test_extend_sensitivity_cpu.py: the CPU
restatement of ``gcv_track_chain`` (include/genconvit_hip.h states the arithmetic: every step is one row of
``gcv_track_match``, so the restatement is a loop over ``followutil.track_match_ref``), a second, independent writing of the
same loop that can be given a defect, and the inputs the GPU test compares on.  No tests here."""
import numpy as np

from tests import followutil as fu
from tests import personutil as pu

NONE = (0, 0, -1, -1)
STOP_NEVER = 2 ** 31 - 1


def track_chain_ref(frames, jobs, grid, radius, max_steps=None):
    """``_lib.track_chain`` on the CPU: int32 (n, max_steps, 4) rows (oy, ox, cost, cost0), ``NONE`` from the step that
    exceeded ``stop``, and from ``steps``, on.  ``jobs``: (n,11) integers (fa, top, right, bottom, left, fs, dir, steps, py, px,
    stop); ``max_steps``: by default the largest ``steps``.  The rows must be valid: this is the restatement, not the
    checks."""
    jobs = np.asarray(jobs, dtype=np.int64).reshape(-1, 11)
    if max_steps is None:
        max_steps = int(jobs[:, 7].max()) if len(jobs) else 0
    out = np.empty((len(jobs), max_steps, 4), dtype=np.int32)
    out[:] = NONE
    for n, (fa, top, right, bottom, left, fs, d, steps, py, px, stop) in enumerate(jobs.tolist()):
        tpl = (fa, top, right, bottom, left)
        t, l, h, w = top + py, left + px, bottom - top, right - left
        for k in range(steps):
            step = fu.track_match_ref(frames, [(fs + d * k, t, l + w, t + h, l, *tpl, 1, *tpl, 0)], grid, radius)[0]
            if int(step[2]) > stop:
                break
            out[n, k] = step
            t, l = t + int(step[0]), l + int(step[1])
    return out


def match_rows(jobs):
    """the ``gcv_track_match`` rows that one-step chains equal: (frame, prior box, template, 1, template, 0)"""
    rows = []
    for fa, top, right, bottom, left, fs, d, steps, py, px, stop in jobs:
        tpl = (fa, top, right, bottom, left)
        rows.append((fs, top + py, right + px, bottom + py, left + px, *tpl, 1, *tpl, 0))
    return rows


# ----------------------------------------------------------------------------- the same loop, written again, with defects
DEFECTS = ("the prior is not advanced", "dir is ignored", "validity at the template's position", "stop compared with >=",
           "the chain goes on after a stop", "cost0 carried over", "(py, px) ignored", "the tie-break is dropped")


def track_chain_alt(frames, jobs, grid, radius, max_steps=None, defect=None):
    """``track_chain_ref`` written a second time, from the header's statement and not through ``track_match_ref`` (all
    candidates of a step at once, through a sliding window over the window cells); ``defect``: None, or one of ``DEFECTS``,
    a way in which a kernel with a step loop could plausibly be wrong."""
    assert defect is None or defect in DEFECTS
    fr = frames.cpu().numpy() if hasattr(frames, "cpu") else np.asarray(frames)
    Y = fu.luma(fr)
    nf, H, W = Y.shape
    G, R = int(grid), int(radius)
    jobs = np.asarray(jobs, dtype=np.int64).reshape(-1, 11)
    if max_steps is None:
        max_steps = int(jobs[:, 7].max()) if len(jobs) else 0
    out = np.empty((len(jobs), max_steps, 4), dtype=np.int32)
    out[:] = NONE
    for n, (fa, top, right, bottom, left, fs, d, steps, py, px, stop) in enumerate(jobs.tolist()):
        h, w = bottom - top, right - left
        ey = lambda u: fu.edge(u, h, G)
        ex = lambda v: fu.edge(v, w, G)
        A = fu._cells(Y[fa], top, left, [ey(u) for u in range(G + 1)], [ex(v) for v in range(G + 1)])
        if defect == "(py, px) ignored":
            py = px = 0
        t, l, carried = top + py, left + px, None
        for k in range(steps):
            f = fs + d * k if defect != "dir is ignored" else min(fs + k, nf - 1)
            inside_y = lambda dd, at: 0 <= at + ey(dd) and at + ey(dd) + h <= H
            inside_x = lambda dd, at: 0 <= at + ex(dd) and at + ex(dd) + w <= W
            vt, vl = (top, left) if defect == "validity at the template's position" else (t, l)
            # (a kernel with that defect would also read outside the frame: here only the candidates it misses count)
            dys = [dd for dd in range(-R, R + 1) if inside_y(dd, vt) and inside_y(dd, t)]
            dxs = [dd for dd in range(-R, R + 1) if inside_x(dd, vl) and inside_x(dd, l)]
            V = fu._cells(Y[f], t, l, [ey(u) for u in range(dys[0], dys[-1] + G + 1)],
                          [ex(v) for v in range(dxs[0], dxs[-1] + G + 1)])
            cost = np.abs(np.lib.stride_tricks.sliding_window_view(V, (G, G)) - A).sum((-1, -2))
            if defect == "the tie-break is dropped":
                best = min((int(cost[i, j]), dy, dx) for i, dy in enumerate(dys) for j, dx in enumerate(dxs))
                c, dy, dx = best
            else:
                c, _, dy, dx = min((int(cost[i, j]), dy * dy + dx * dx, dy, dx) for i, dy in enumerate(dys)
                                   for j, dx in enumerate(dxs))
            cost0 = int(cost[dys.index(0), dxs.index(0)])
            shown = carried if defect == "cost0 carried over" and carried is not None else cost0
            carried = cost0
            if c >= stop if defect == "stop compared with >=" else c > stop:
                if defect == "the chain goes on after a stop":
                    continue
                break
            out[n, k] = (ey(dy), ex(dx), c, shown)
            if defect != "the prior is not advanced":
                t, l = t + ey(dy), l + ex(dx)
    return out


# ----------------------------------------------------------------------------- the material cost_max's default is read from
POLICY_PATTERNS, POLICY_FRAMES, POLICY_GONE = 6, 8, 5        # per video: the pattern is there in frames 0 ... 4, gone from 5


def policy_video(ident, grid):
    """(frames, job, truth): 8 frames of 200 x 280 of the drifting background; the smooth pattern ``ident``, 64 ... 120
    pixels a side, moves by up to 3 cells of the grid a frame (any number of pixels, not whole cells) under pixel noise of
    sigma 3, a new draw every frame, and is removed from frame 5 on.  ``job``: the chain from frame 0 over the 7 others;
    ``truth``: the pattern's (top, left) in frames 0 ... 4."""
    r = np.random.default_rng(500 + 10 * ident + grid)
    H, W = 200, 280
    h, w = int(r.integers(64, 121)), int(r.integers(64, 121))
    frames = fu.background(POLICY_FRAMES, H, W)
    t, l = (H - h) // 2, (W - w) // 2
    truth = []
    for f in range(POLICY_GONE):
        if f:
            t = int(np.clip(t + r.uniform(-3, 3) * h / grid, 0, H - h))
            l = int(np.clip(l + r.uniform(-3, 3) * w / grid, 0, W - w))
        frames[f, t:t + h, l:l + w] = pattern(ident, h, w, sigma=3.0, noise_seed=1 + 100 * ident + 10 * grid + f)
        truth.append((t, l))
    t, l = truth[0]
    return frames, (0, t, l + w, t + h, l, 1, 1, POLICY_FRAMES - 1, 0, 0, STOP_NEVER), truth


def policy_costs(radius=8):
    """(largest cost per cell of a step that still follows the pattern, smallest cost per cell of a step after the pattern
    is gone) over ``POLICY_PATTERNS`` patterns at grids 16, 32 and 64.  A step follows when its box is within one cell of
    the truth in both directions."""
    follows, gone = [], []
    for grid in (16, 32, 64):
        for ident in range(POLICY_PATTERNS):
            frames, job, truth = policy_video(ident, grid)
            h, w = job[3] - job[1], job[2] - job[4]
            out = track_chain_alt(frames, [job], grid, radius)[0]
            t, l = job[1], job[4]
            for k, (oy, ox, cost, _) in enumerate(out.tolist()):
                t, l = t + oy, l + ox
                if k + 1 < POLICY_GONE:
                    assert abs(t - truth[k + 1][0]) <= h / grid + 1 and abs(l - truth[k + 1][1]) <= w / grid + 1, (grid, ident, k)
                    follows.append(cost / (grid * grid))
                else:
                    gone.append(cost / (grid * grid))
    return max(follows), min(gone)


# ----------------------------------------------------------------------------- the inputs of the GPU test
def pattern(seed, h, w, sigma=0.0, noise_seed=0):
    """a smooth random colour pattern of tests/personutil.py at h x w pixels"""
    return pu.shot(pu.identity(seed), h, w, sigma=sigma, seed=noise_seed)


MOVE_H, MOVE_W = 48, 40
MOVE_PATH = [(20, 0), (23, 9), (29, 21), (31, 26), (26, 18), (22, 6)]          # (top, left) in frames 0 ... 5


def moving_case():
    """(frames, jobs, grid, radius): 6 frames of 96 x 128, a smooth 48 x 40 pattern on ``MOVE_PATH`` over the drifting
    background — from the left border to the right and back, a different displacement at every step — followed forward
    from frame 0 and backward from frame 5.  At the left border the template's position allows no step to the left, the
    later priors do."""
    frames = fu.background(6, 96, 128)
    patch = pattern(11, MOVE_H, MOVE_W)
    for f, (t, l) in enumerate(MOVE_PATH):
        frames[f, t:t + MOVE_H, l:l + MOVE_W] = patch
    box = lambda f: (f, MOVE_PATH[f][0], MOVE_PATH[f][1] + MOVE_W, MOVE_PATH[f][0] + MOVE_H, MOVE_PATH[f][1])
    jobs = [(*box(0), 1, 1, 5, 0, 0, STOP_NEVER), (*box(5), 4, -1, 5, 0, 0, STOP_NEVER)]
    return frames, jobs, 16, 5


def split(jobs, first, offsets):
    """the two launches that equal one: ``first`` steps of every job, and the rest from ``offsets[n]`` = the sum of the
    (oy, ox) of job n's first launch"""
    head = [(*j[:7], first, *j[8:]) for j in jobs]
    tail = [(*j[:5], j[5] + j[6] * first, j[6], j[7] - first, j[8] + int(o[0]), j[9] + int(o[1]), j[10])
            for j, o in zip(jobs, offsets)]
    return head, tail


def stop_case():
    """(frames, jobs, grid, radius): 6 frames of 96 x 128 with a smooth pattern that moves a little, is missing in frame 3
    and back in frames 4 and 5; five-step chains from frame 0.  The first never stops.  The others' ``stop`` is set from
    that one's costs c[k] (this file's restatement gives them): max(c[0], c[1]) <= stop < c[2] stops in the middle, at the
    frame without the pattern, although frames 4 and 5 would match again; stop = c[2] exactly does not stop (> and not
    >=); stop = c[0] - 1 stops at once."""
    frames = fu.background(6, 96, 128)
    patch = pattern(12, 40, 44)
    for f, (t, l) in {0: (30, 40), 1: (32, 43), 2: (33, 47), 4: (35, 52), 5: (34, 55)}.items():
        frames[f, t:t + 40, l:l + 44] = patch
    job = lambda stop: (0, 30, 84, 70, 40, 1, 1, 5, 0, 0, stop)
    c = track_chain_ref(frames, [job(STOP_NEVER)], 16, 4)[0, :, 2].tolist()
    assert max(c[0], c[1]) < c[2] and max(c[3], c[4]) < c[2] and c[0] >= 1
    jobs = [job(STOP_NEVER), job(max(c[0], c[1])), job(c[2] - 1), job(c[2]), job(c[0] - 1), job(0)]
    return frames, jobs, 16, 4


def border_case():
    """(frames, jobs, grid, radius): 5 frames of 96 x 128, a smooth pattern that runs into the bottom right corner (the last
    two positions would leave the frame: the pattern is cut off there), so that the valid candidates shrink from step to
    step; followed from frame 0 at radius 8, and once more from a template that touches the corner already."""
    frames = fu.background(5, 96, 128)
    patch = pattern(13, 36, 34)
    for f, (t, l) in enumerate([(40, 70), (48, 80), (55, 88), (62, 97), (70, 105)]):
        part = patch[:96 - t, :128 - l]
        frames[f, t:t + part.shape[0], l:l + part.shape[1]] = part
    jobs = [(0, 40, 104, 76, 70, 1, 1, 4, 0, 0, STOP_NEVER), (2, 55, 122, 91, 88, 3, 1, 2, 5, 6, STOP_NEVER),
            (0, 40, 104, 76, 70, 4, -1, 4, 20, 24, STOP_NEVER)]
    return frames, jobs, 16, 8


def random_case(grid, nf=6, H=120, W=160, n=48, hi=100, seed=29, max_len=5):
    """(frames, jobs): ``nf`` frames of H x W — noise, but frame 2 flat (every candidate costs the same: ties) and frame 4
    smooth — and ``n`` random chains: sides grid ... hi that are no multiple of 16, both directions, 1 ... ``max_len`` steps
    mixed in one launch, a first prior off the template by up to 6 pixels, templates that touch each border, and a
    ``stop`` that for a third of the jobs is low enough to end some chains."""
    rng = np.random.default_rng(seed + grid)
    frames = rng.integers(0, 256, (nf, H, W, 3), dtype=np.uint8)
    frames[2] = (90, 140, 60)
    if nf > 4:
        y, x = np.mgrid[0:H, 0:W]
        frames[4] = np.stack([(3 * y + x) % 256, (2 * x + y) % 256, (y * x // 7) % 256], -1).astype(np.uint8)

    def side(top):
        while True:
            s = int(rng.integers(grid, top + 1))
            if s % 16 or grid == top:
                return s
    jobs = []
    for i in range(n):
        h, w = side(min(hi, H)), side(min(hi, W))
        top, left = int(rng.integers(0, H - h + 1)), int(rng.integers(0, W - w + 1))
        where = ("top", "bottom", "left", "right")[i % 8] if i % 8 < 4 else None
        top = {"top": 0, "bottom": H - h}.get(where, top)
        left = {"left": 0, "right": W - w}.get(where, left)
        d = 1 if rng.integers(0, 2) else -1
        steps = int(rng.integers(1, max_len + 1))
        fs = int(rng.integers(0, nf - steps + 1)) if d == 1 else int(rng.integers(steps - 1, nf))
        py = int(np.clip(rng.integers(-6, 7), -top, H - h - top))
        px = int(np.clip(rng.integers(-6, 7), -left, W - w - left))
        stop = int(rng.integers(4, 50)) * grid * grid if i % 3 == 0 else STOP_NEVER
        jobs.append((int(rng.integers(0, nf)), top, left + w, top + h, left, fs, d, steps, py, px, stop))
    return frames, jobs


def large_case():
    """(frames, jobs, grid, radius): the largest configuration, grid 64 with radius 32, on three-step chains: 3 x 256 x 256
    frames and boxes of 64 ... 120 a side, sized as followutil.fuzz_case's largest"""
    frames, jobs = random_case(64, nf=3, H=256, W=256, n=8, hi=120, seed=31, max_len=3)
    jobs = [(*j[:5], 0 if j[6] == 1 else 2, j[6], 3, *j[8:]) for j in jobs]
    return frames, jobs, 64, 32
