"""Helpers of tests/test_persons_cpu.py, tests/test_persons_sensitivity_cpu.py and tests/test_persons_gpu.py: the CPU
restatements of ``gcv_face_signature`` and ``gcv_sig_link`` (include/genconvit_hip.h states the arithmetic; this file is
written from that statement, in numpy int64) and the synthetic material the tests tell apart: smooth random colour
patterns ("identities"), seen again under another gain, offset, shift, box size and noise ("shots").  No tests here."""
import numpy as np

from tests import followutil as fu

NONE = 0xFFFFFFFF                                            # no pair of rows: the diagonal, a track without rows
SIG_BYTES = 384


# ----------------------------------------------------------------------------- gcv_face_signature
def edges(extent, grid):
    """e[i] = (i extent) >> log2(grid), i = 0 ... grid"""
    return np.array([(i * int(extent)) // grid for i in range(grid + 1)], dtype=np.int64)


def cell_sums(plane, box, ey, ex):
    """(sums, counts) of the int64 ``plane`` over the cells rows [top + ey[u], top + ey[u + 1]) x columns [left + ex[v],
    left + ex[v + 1]) of ``box`` = (top, right, bottom, left); the cells are not empty and lie inside the plane"""
    top, right, bottom, left = (int(v) for v in box)
    ys, xs = ey + top, ex + left
    assert ys[0] >= 0 and xs[0] >= 0 and ys[-1] <= plane.shape[0] and xs[-1] <= plane.shape[1]
    assert (np.diff(ys) > 0).all() and (np.diff(xs) > 0).all()
    region = np.asarray(plane, dtype=np.int64)[ys[0]:ys[-1], xs[0]:xs[-1]]
    sums = np.add.reduceat(np.add.reduceat(region, ys[:-1] - ys[0], axis=0), xs[:-1] - xs[0], axis=1)
    return sums, np.diff(ys)[:, None] * np.diff(xs)[None, :]


def rounded_mean(sums, cnt):
    return (sums + cnt // 2) // cnt


def chroma(frame):
    """(Cb, Cr) planes of a uint8 (H, W, 3) frame, int64: 1 ... 256"""
    f = np.asarray(frame).astype(np.int64)
    r, g, b = f[..., 0], f[..., 1], f[..., 2]
    return (32896 - 43 * r - 85 * g + 128 * b) >> 8, (32896 + 128 * r - 107 * g - 21 * b) >> 8


def normalise(c):
    """N of the (16, 16) cell values c: clamp(128 + sgn(d) ((8192 |d| + A // 2) // A), 0, 255) with d = 256 c - S1 and
    A = sum |d|; 128 everywhere when A == 0.  int64"""
    c = np.asarray(c, dtype=np.int64)
    d = 256 * c - c.sum()
    A = int(np.abs(d).sum())
    if A == 0:
        return np.full_like(c, 128)
    return np.clip(128 + np.sign(d) * ((8192 * np.abs(d) + A // 2) // A), 0, 255)


def signature_of(frame, box, edges=edges, mean=rounded_mean, normalise=normalise, chroma=chroma):
    """The 384 bytes of one box = (top, right, bottom, left) of one uint8 (H, W, 3) frame.  The pieces are arguments so that
    tests/test_persons_sensitivity_cpu.py can plant a wrong one; nobody else passes them."""
    top, right, bottom, left = (int(v) for v in box)
    h, w = bottom - top, right - left
    assert h >= 16 and w >= 16
    luma = mean(*cell_sums(fu.luma(frame), box, edges(h, 16), edges(w, 16)))
    cb, cr = chroma(frame)
    ey, ex = edges(h, 8), edges(w, 8)
    cells = [np.minimum(mean(*cell_sums(plane, box, ey, ex)), 255) for plane in (cb, cr)]
    row = np.concatenate([normalise(luma).reshape(-1), cells[0].reshape(-1), cells[1].reshape(-1)])
    return (row & 0xFF).astype(np.uint8)                     # a wrong piece may leave the byte range; the right ones do not


def face_signature_ref(frames, boxes, **pieces):
    """``_lib.face_signature`` on the CPU: uint8 (n,384).  ``frames``: uint8 (F,H,W,3), numpy or tensor; ``boxes``: (n,5)
    integers.  The rows must be valid (inside the frame, every side >= 16): this is the restatement, not the checks."""
    fr = frames.cpu().numpy() if hasattr(frames, "cpu") else np.asarray(frames)
    boxes = np.asarray(boxes, dtype=np.int64).reshape(-1, 5)
    out = np.zeros((len(boxes), SIG_BYTES), dtype=np.uint8)
    for n, (f, *box) in enumerate(boxes.tolist()):
        out[n] = signature_of(fr[f], box, **pieces)
    return out


# ----------------------------------------------------------------------------- gcv_sig_link
def sig_link_ref(sig, owner, tracks, chunk=16):
    """``_lib.sig_link`` on the CPU: int64 (T,T); out[a][b], a != b, = min over rows i of track a and j of track b of
    sum_k |sig[i][k] - sig[j][k]|; ``NONE`` on the diagonal and where a track has no row.  Rows whose owner is -1 take no
    part."""
    sig = np.asarray(sig.cpu() if hasattr(sig, "cpu") else sig, dtype=np.uint8).reshape(-1, SIG_BYTES)
    owner = np.asarray(owner, dtype=np.int64).reshape(-1)
    T = int(tracks)
    assert len(owner) == len(sig) and ((owner >= -1) & (owner < T)).all()
    out = np.full((T, T), NONE, dtype=np.int64)
    rows = np.nonzero(owner >= 0)[0]
    rows = rows[np.argsort(owner[rows], kind="stable")]      # by track: the rows of a track are one run
    if len(rows) == 0:
        return out
    s, o = sig[rows].astype(np.int16), owner[rows]
    present, starts = np.unique(o, return_index=True)
    for lo in range(0, len(rows), chunk):
        d = np.abs(s[lo:lo + chunk, None, :] - s[None, :, :]).sum(-1, dtype=np.int64)       # (chunk, rows)
        best = np.minimum.reduceat(d, starts, axis=1)                                        # per row, per present track
        for k in range(best.shape[0]):
            out[o[lo + k], present] = np.minimum(out[o[lo + k], present], best[k])
    out[np.arange(T), np.arange(T)] = NONE
    return out


# ----------------------------------------------------------------------------- synthetic identities
def identity(seed, knots=7):
    """A smooth random colour pattern: (knots, knots, 3) float64 control values in [30, 225], read bilinearly"""
    return np.random.default_rng(1000 + seed).uniform(30.0, 225.0, (knots, knots, 3))


def shot(pattern, h, w, gain=1.0, offset=0.0, shift=(0.0, 0.0), sigma=0.0, seed=0):
    """uint8 (h, w, 3): the pattern at h x w pixels, moved by ``shift`` = (dy, dx) pixels, as gain * value + offset plus
    Gaussian noise of ``sigma``, rounded and clipped"""
    k = pattern.shape[0]
    y = np.clip((np.arange(h) + 0.5 + shift[0]) / h, 0.0, 1.0) * (k - 1)
    x = np.clip((np.arange(w) + 0.5 + shift[1]) / w, 0.0, 1.0) * (k - 1)
    y0, x0 = np.minimum(y.astype(int), k - 2), np.minimum(x.astype(int), k - 2)
    fy, fx = (y - y0)[:, None, None], (x - x0)[None, :, None]
    p = pattern
    img = (p[y0][:, x0] * (1 - fy) * (1 - fx) + p[y0][:, x0 + 1] * (1 - fy) * fx + p[y0 + 1][:, x0] * fy * (1 - fx) +
           p[y0 + 1][:, x0 + 1] * fy * fx)
    img = gain * img + offset
    if sigma:
        img = img + np.random.default_rng(seed).normal(0.0, sigma, img.shape)
    return np.clip(np.rint(img), 0, 255).astype(np.uint8)


IDENTITIES, SHOTS = 6, 6                                     # the material link_max's default is read from


def shot_params(ident, k):
    """the k-th shot of an identity: box sides 64 ... 200, gain 0.8 ... 1.15, offset +-20, shifts of up to 3 pixels, sigma 3"""
    r = np.random.default_rng(77 * ident + k)
    return dict(h=int(r.integers(64, 201)), w=int(r.integers(64, 201)), gain=float(r.uniform(0.8, 1.15)),
                offset=float(r.uniform(-20, 20)), shift=(float(r.uniform(-3, 3)), float(r.uniform(-3, 3))), sigma=3.0,
                seed=1 + 100 * ident + k)


def identity_distances():
    """(largest distance between two shots of one identity, smallest between shots of two) over ``IDENTITIES`` patterns of
    ``SHOTS`` shots each, every shot a whole frame of its own"""
    sigs, who = [], []
    for ident in range(IDENTITIES):
        for k in range(SHOTS):
            img = shot(identity(ident), **shot_params(ident, k))
            sigs.append(signature_of(img, (0, img.shape[1], img.shape[0], 0)).astype(np.int64))
            who.append(ident)
    sigs, who = np.stack(sigs), np.array(who)
    d = np.abs(sigs[:, None, :] - sigs[None, :, :]).sum(-1)
    same = who[:, None] == who[None, :]
    return int(d[same].max()), int(d[~same].min())


FACE = (24, 84, 72, 40)                                      # (top, right, bottom, left): 48 x 44 pixels
SHOT_FRAMES = 4
CUTS = [4, 8, 12]                                            # four shots of four frames: identities 0, 1, 0, 1


def interview():
    """(frames, detections, cuts): 16 frames of 96 x 128, four shots that cut between two identities in (nearly) the same
    box — position alone would make one track of it.  Every shot has its own gain, offset, background and box (a few
    pixels off ``FACE``), every frame its own noise.  ``detections``: rows (frame, top, right, bottom, left)."""
    frames = np.zeros((4 * SHOT_FRAMES, 96, 128, 3), dtype=np.uint8)
    det = []
    looks = [(1.0, 0.0, (0, 0, 0, 0), 90), (0.9, 12.0, (2, 1, 3, -2), 140), (1.12, -15.0, (-3, 4, -1, 2), 60),
             (0.85, 18.0, (1, -3, 4, 3), 110)]
    for s, (gain, offset, (dt, dr, db, dl), grey) in enumerate(looks):
        top, right, bottom, left = FACE[0] + dt, FACE[1] + dr, FACE[2] + db, FACE[3] + dl
        for k in range(SHOT_FRAMES):
            f = s * SHOT_FRAMES + k
            frames[f] = grey
            frames[f, top:bottom, left:right] = shot(identity(s % 2), bottom - top, right - left, gain, offset,
                                                     shift=(0.5 * k, -0.5 * k), sigma=3.0, seed=500 + f)
            det.append((f, top, right, bottom, left))
    return frames, det, list(CUTS)


TWIN_A, TWIN_B = (10, 60, 58, 16), (40, 120, 88, 76)         # two boxes of 48 x 44 that never overlap


def twins():
    """(frames, detections): 6 frames of 96 x 128 with the SAME identity in two places of every frame (noise apart): as
    alike as two faces get, and two people all the same"""
    frames = np.full((6, 96, 128, 3), 100, dtype=np.uint8)
    det = []
    for f in range(6):
        for n, (top, right, bottom, left) in enumerate((TWIN_A, TWIN_B)):
            frames[f, top:bottom, left:right] = shot(identity(3), bottom - top, right - left, sigma=2.0, seed=900 + 2 * f + n)
            det.append((f, top, right, bottom, left))
    return frames, det


# ----------------------------------------------------------------------------- the inputs of the GPU tests
def signature_case():
    """(frames, boxes) of tests/test_persons_gpu.py: 5 frames of 96 x 128 — three of random bytes, a flat one, and one of
    stripes (left half black with a white stripe of 4 pixels every 64, right half the inverse) — and boxes of side 16
    (cells of one pixel), 17 x 23 (uneven cells), 16 x 100, 90 x 16, the whole frame, one touching each border, one on the
    flat frame (A = 0) and two on the stripes, whose few bright (dark) cells clamp at 255 (0)."""
    frames = np.random.default_rng(41).integers(0, 256, (5, 96, 128, 3), dtype=np.uint8)
    frames[3] = (10, 200, 30)
    x = np.arange(128)
    white = np.where(x < 64, x % 64 < 4, x % 64 >= 4)
    frames[4] = np.where(white, 255, 0).astype(np.uint8)[None, :, None]
    boxes = [(0, 5, 23, 21, 7), (1, 40, 53, 57, 30), (2, 3, 111, 19, 11), (0, 2, 37, 92, 21), (1, 0, 128, 96, 0),
             (2, 0, 128, 96, 0), (0, 0, 60, 31, 20), (1, 30, 128, 70, 77), (2, 61, 90, 96, 40), (0, 33, 45, 80, 0),
             (3, 10, 100, 70, 20), (3, 0, 128, 96, 0), (4, 10, 64, 74, 0), (4, 20, 128, 84, 64), (4, 0, 128, 96, 0)]
    return frames, boxes


def link_cases():
    """[(name, sig uint8 (n,384), owner (n,), T)] of tests/test_persons_gpu.py: random signatures around every edge of the
    64-row tiles, unsorted owners, rows that take no part, a track without rows, T = 1, equal rows and the largest distance"""
    rng = np.random.default_rng(43)
    rand = lambda n: rng.integers(0, 256, (n, SIG_BYTES), dtype=np.uint8)

    def near(sig, row, other):
        """``row`` becomes ``other`` but for four bytes: the pair decides the minimum of its two tracks (distance 4 * 255)"""
        sig[row] = sig[other]
        sig[row, :4] ^= 0xFF
        return sig
    cases = [("n=1", rand(1), [0], 2)]
    for n in (63, 64, 65):                                   # the LAST row (alone in its tile at n = 65) decides out[0][2]
        cases.append((f"n={n}", near(rand(n), n - 1, 0), [(3 * i) // n for i in range(n)], 3))
    bounds = [0, 7, 61, 70, 127, 130]                        # five tracks; their boundaries fall inside the tiles
    sorted_owner = [t for t in range(5) for _ in range(bounds[t + 1] - bounds[t])]
    s130 = near(rand(130), 129, 1)                           # the last row of the last, partial tile decides out[0][4]
    cases.append(("n=130", s130, sorted_owner, 5))
    perm = [int(i) for i in rng.permutation(130) if i != 129] + [129]                       # ... also where the rows are shuffled
    cases.append(("unsorted", s130[perm], [sorted_owner[i] for i in perm], 5))
    out = [(-1 if i % 3 == 0 else o) for i, o in enumerate(sorted_owner)]
    out[128] = out[129] = 4                                  # the last tile keeps rows, and row 64 ... too
    cases.append(("owner -1", s130, out, 5))
    cases.append(("empty track", rand(70), [(0, 1, 3)[i % 3] for i in range(70)], 4))           # track 2 has no row
    cases.append(("T=1", rand(5), [0] * 5, 1))
    twin = rand(66)
    twin[65] = twin[2]
    cases.append(("equal rows", twin, [0] * 33 + [1] * 33, 2))
    far = np.zeros((3, SIG_BYTES), dtype=np.uint8)
    far[1:] = 255
    cases.append(("0 against 255", far, [0, 1, 1], 2))
    return cases
