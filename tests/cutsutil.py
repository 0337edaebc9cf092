"""Helpers of tests/test_cuts_cpu.py and tests/test_cuts_gpu.py: the CPU restatement of ``gcv_frame_hist`` and
``gcv_hist_diff`` (include/genconvit_hip.h states the arithmetic; this file is written from that statement, with
``np.bincount`` on slices), of the score ``pred_func.shot_cuts`` derives from them, and the synthetic videos.  No tests
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
