"""Helpers of tests/test_cuts_cpu.py, tests/test_cuts_gpu.py and tests/test_cuts_sensitivity_cpu.py: the CPU restatement of
``gcv_frame_hist`` and ``gcv_hist_diff`` (include/genconvit_hip.h states the arithmetic; this file is written from that
statement, with ``np.bincount`` on slices), of the score ``pred_func.shot_cuts`` derives from them, a second writing of both
entries that can be given a defect (with the launch's split into row slices restated), and the synthetic videos.  No tests
here."""
import numpy as np
import torch

BINS = 64


def luma(frames):
    """Y = (77 R + 150 G + 29 B + 128) >> 8 of uint8 (..., 3) pixels, int64."""
    f = np.asarray(frames).astype(np.int64)
    return (77 * f[..., 0] + 150 * f[..., 1] + 29 * f[..., 2] + 128) >> 8


def edges(extent, regions):
    """[(u * extent) // regions for u = 0 ... regions]"""
    return [(u * int(extent)) // int(regions) for u in range(int(regions) + 1)]


def region_pixels(H, W, regions):
    """pixel count of region u * regions + v, int64 (regions^2,)"""
    ey, ex = edges(H, regions), edges(W, regions)
    return np.array([(ey[u + 1] - ey[u]) * (ex[v + 1] - ex[v]) for u in range(regions) for v in range(regions)],
                    dtype=np.int64)


def _numpy(frames):
    return frames.cpu().numpy() if hasattr(frames, "cpu") else np.asarray(frames)


def frame_hist_ref(frames, regions):
    """``_lib.frame_hist`` on the CPU: int32 (F, regions^2, 64).  ``frames``: uint8 (F,H,W,3), numpy or tensor."""
    fr = _numpy(frames)
    bins = luma(fr) >> 2
    F, H, W = bins.shape
    ey, ex = edges(H, regions), edges(W, regions)
    out = np.zeros((F, regions * regions, BINS), dtype=np.int32)
    for f in range(F):
        for u in range(regions):
            for v in range(regions):
                out[f, u * regions + v] = np.bincount(bins[f, ey[u]:ey[u + 1], ex[v]:ex[v + 1]].ravel(), minlength=BINS)
    return out


def hist_diff_ref(hist):
    """``_lib.hist_diff`` on the CPU: int64 (F - 1, regions^2) — the one value that does not fit int32 is 2^31."""
    h = _numpy(hist).astype(np.int64)
    return np.abs(h[1:] - h[:-1]).sum(-1)


def scores_ref(dist, H, W, regions):
    """The score of every pair of consecutive frames, float64 (F - 1,): of the regions^2 regions keep the max(1, regions^2
    // 2) with the smallest (dist, r); sum of their dist / (2 * sum of their pixel counts)."""
    n = region_pixels(H, W, regions)
    keep = max(1, regions * regions // 2)
    out = []
    for row in np.asarray(dist).tolist():
        kept = sorted((int(d), r) for r, d in enumerate(row))[:keep]
        out.append(sum(d for d, _ in kept) / (2 * sum(int(n[r]) for _, r in kept)))
    return np.array(out, dtype=np.float64)


# ----------------------------------------------------------------------------- the device entries on the CPU
def frame_hist_cpu(frames_u8, regions=4, out=None):
    """stands in for ``_lib.frame_hist`` where there is no GPU: host tensors in, host tensors out"""
    hist = torch.as_tensor(frame_hist_ref(frames_u8, regions))
    if out is None:
        return hist
    out.copy_(hist)
    return out


def hist_diff_cpu(hist):
    return torch.as_tensor(hist_diff_ref(hist).astype(np.int32))


# ----------------------------------------------------------------------------- videos
SHOTS = (5, 4, 6)                                          # frames per shot: new shots start at frames 5 and 9
CUTS = [5, 9]
FACE_BOX = (20, 90, 80, 30)                                # (top, right, bottom, left): the box a "face" keeps across both cuts
SKIN = (224, 172, 140)


def three_shot_video(seed=5):
    """15 x 90 x 130 frames in shots of 5, 4 and 6: a dark horizontal ramp, a brighter vertical ramp whose luma range
    overlaps the first one's, and a checker of 13-pixel squares — each with fresh +-6 noise per channel on every frame —
    and a 36 x 30 skin-coloured patch that moves by (3, 5) pixels a frame inside every shot.  3 * 130 = 390 bytes a row is
    no multiple of 4, and 90 and 130 are divisible by neither 4 nor 8.
    With the restatement at regions = 4 (tests/test_cuts_cpu.py asserts the bounds): the 12 scores inside a shot lie in
    0.018 ... 0.040 and the two cuts score 0.966 and 0.925."""
    rng = np.random.default_rng(seed)
    H, W = 90, 130
    y, x = np.mgrid[0:H, 0:W]
    zero = np.zeros((H, W))
    looks = [
        np.stack((50 + 40 * x / W, 70 + 30 * x / W, 90 + zero), -1),
        np.stack((90 + 50 * y / H, 100 + 60 * y / H, 80 + 40 * y / H), -1),
        np.where((((y // 13) + (x // 13)) % 2 == 0)[..., None], np.array([60.0, 110.0, 70.0]), np.array([170.0, 150.0, 200.0])),
    ]
    frames = []
    for look, n, (py, px) in zip(looks, SHOTS, ((6, 10), (40, 70), (20, 40))):
        for k in range(n):
            fr = look + rng.integers(-6, 7, size=(H, W, 3))
            fr[py + 3 * k:py + 3 * k + 36, px + 5 * k:px + 5 * k + 30] = SKIN
            frames.append(np.clip(fr, 0, 255).astype(np.uint8))
    return np.stack(frames)


def noise_video(F=4, H=37, W=53, seed=11):
    """uniform noise: every bin of every region is hit, the regions at R = 8 are 4-5 x 6-7 pixels"""
    return np.random.default_rng(seed).integers(0, 256, size=(F, H, W, 3), dtype=np.uint8)


def flat_pair(side=260):
    """two frames, flat 200 and flat 17: one bin holds side^2 pixels, and the histograms are disjoint"""
    fr = np.empty((2, side, side, 3), dtype=np.uint8)
    fr[0], fr[1] = 200, 17
    return fr


def striped_pair(H=64, W=96):
    """columns alternate between two values (the neighbouring lanes of a wave hit two bins in turn), then between two
    others"""
    fr = np.empty((2, H, W, 3), dtype=np.uint8)
    fr[0, :, 0::2], fr[0, :, 1::2] = 40, 41
    fr[1, :, 0::2], fr[1, :, 1::2] = 40, 250
    return fr


def many_video():
    """70 frames of 37 x 53 noise: at R = 4 they are 1 120 regions, more than the 1 024 the launcher splits below"""
    return noise_video(F=70, seed=12)


def tiny_video():
    """2 x 8 x 8 noise: at R = 8 a region is one pixel"""
    return noise_video(F=2, H=8, W=8, seed=13)


def ends_pair(H=16, W=24):
    """two frames that fill the first and the last bin: white, then black with every third column white — bin 63 is the last
    lane of ``hist_diff``'s wave, and noise almost never reaches it (Y >= 252)"""
    fr = np.zeros((2, H, W, 3), dtype=np.uint8)
    fr[0] = 255
    fr[1, :, 0::3] = 255
    return fr


# ----------------------------------------------------------------------------- the launch's split, restated
FH_TARGET_WGS = 1024                                       # csrc/cuts.hip: split until about 4 workgroups a CU exist ...
FH_MIN_ROWS = 8                                            # ... but leave every slice at least 8 pixel rows


def launch_slices(units, rows_each):
    """S of ``launch_frame_hist`` (units = frames x regions^2, rows_each = H // regions) and of ``launch_frame_cells``
    (units = frames x grid, rows_each = H // grid): the row slices a region or a row of cells is split into"""
    if units >= FH_TARGET_WGS:
        return 1
    return min(-(-FH_TARGET_WGS // units), max(1, rows_each // FH_MIN_ROWS))


def hist_slices(nframes, H, regions):
    return launch_slices(nframes * regions * regions, H // regions)


def slice_rows(y0, y1, S, defect=None):
    """multiplicity of the pixel rows y0 ... y1 - 1 of a region (or row of cells) over its S slices [y0 + s n // S,
    y0 + (s + 1) n // S): 1 each, but with "counted twice" every slice except the last also takes the first row of the next,
    and with "dropped" it leaves out its own last row."""
    n = y1 - y0
    mult = np.zeros(n, dtype=np.int64)
    for s in range(S):
        a, b = s * n // S, (s + 1) * n // S
        if s < S - 1:
            b += {"twice": 1, "dropped": -1}.get(defect, 0)
        mult[a:max(a, b)] += 1
    return mult


# ----------------------------------------------------------------------------- the same entries, written again, with defects
HIST_DEFECTS = ("luma without rounding", "region edges rounded", "regions transposed", "a row's last partial group dropped",
                "a row's last partial group counted as four pixels", "the byte-wise groups dropped",
                "the slice-boundary row counted twice", "the slice-boundary row dropped", "counts truncated to 16 bits")
DIFF_DEFECTS = ("bin 63 left out of the distance", "a - b without the absolute value",
                "the second frame lag regions on", "lag ignored")


def frame_hist_alt(frames, regions, defect=None):
    """``frame_hist_ref`` written a second time, the way csrc/cuts.hip walks a frame: per region a map of how often each
    pixel is counted (rows by slice, columns by 4-pixel group), and one weighted bincount per frame and region.  ``defect``:
    None or one of ``HIST_DEFECTS``.  "counted as four pixels" counts the pixels right of the region in the same pixel row;
    where that passes the row's end a kernel would go on in the next row, here they are left out (it differs long before).
    "the byte-wise groups dropped": the first group of frame 0 and the last group of the last frame, which the kernel
    reads byte by byte because the aligned dwords around them start before or end behind the buffer."""
    assert defect is None or defect in HIST_DEFECTS, defect
    fr = _numpy(frames)
    f = fr.astype(np.int64)
    bins = (77 * f[..., 0] + 150 * f[..., 1] + 29 * f[..., 2] + (0 if defect == "luma without rounding" else 128)) >> 10
    F, H, W = bins.shape
    R = int(regions)
    half = R // 2 if defect == "region edges rounded" else 0
    ey, ex = [(u * H + half) // R for u in range(R + 1)], [(v * W + half) // R for v in range(R + 1)]
    S = hist_slices(F, H, R)
    out = np.zeros((F, R * R, BINS), dtype=np.int64)
    for u in range(R):
        rows = slice_rows(ey[u], ey[u + 1], S, {"the slice-boundary row counted twice": "twice",
                                                "the slice-boundary row dropped": "dropped"}.get(defect))
        for v in range(R):
            x0, x1 = ex[v], ex[v + 1]
            w = x1 - x0
            cols = np.zeros(W, dtype=np.int64)
            cols[x0:x1] = 1
            if defect == "a row's last partial group dropped" and w % 4:
                cols[x1 - w % 4:x1] = 0
            if defect == "a row's last partial group counted as four pixels" and w % 4:
                cols[x1:min(W, x1 + 4 - w % 4)] += 1
            m = np.zeros((H, W), dtype=np.int64)
            m[ey[u]:ey[u + 1]] = rows[:, None] * cols[None, :]
            r = v * R + u if defect == "regions transposed" else u * R + v
            for k in range(F):
                mk = m
                if defect == "the byte-wise groups dropped" and ((k == 0 and u == v == 0) or (k == F - 1 and u == v == R - 1)):
                    mk = m.copy()
                    if k == 0 and u == v == 0:
                        mk[ey[0], x0:x0 + 4] = 0
                    if k == F - 1 and u == v == R - 1:
                        mk[H - 1, x0 + 4 * ((w - 1) // 4):] = 0
                out[k, r] = np.bincount(bins[k].ravel(), weights=mk.ravel(), minlength=BINS).astype(np.int64)
    if defect == "counts truncated to 16 bits":
        out &= 0xFFFF
    return out.astype(np.int32)


def hist_diff_alt(hist, lag=1, defect=None):
    """``hist_diff_ref`` / ``transutil.hist_diff_lag_ref`` written a second time, as the kernel indexes: item = pair *
    regions^2 + region against item + lag * regions^2 of the flat histograms, in 32-bit arithmetic; int64 of the int32 the
    entry returns.  ``defect``: None or one of ``DIFF_DEFECTS``."""
    assert defect is None or defect in DIFF_DEFECTS, defect
    h = _numpy(hist).astype(np.int64)
    F, RR, _ = h.shape
    flat = h.reshape(F * RR, BINS)
    items = max(0, F - lag) * RR
    step = {"the second frame lag regions on": lag, "lag ignored": RR}.get(defect, lag * RR)
    a, b = flat[:items], flat[step:step + items]
    d = (a - b) % 2 ** 32 if defect == "a - b without the absolute value" else np.abs(a - b)
    if defect == "bin 63 left out of the distance":
        d = d[:, :BINS - 1]
    return (d.sum(-1) % 2 ** 32).astype(np.uint32).view(np.int32).astype(np.int64).reshape(max(0, F - lag), RR)
