"""Helpers of tests/test_scan_cpu.py and tests/test_scan_gpu.py: CPU restatements of the two device entry points behind
``pred_func.scan_frames`` (``gcv_vote_windows``, ``gcv_face_crop_preprocess``) and shared inputs.  No tests here."""
import numpy as np
import torch


def vote_windows_ref(logits, batch, nets, ranges):
    """``_lib.vote_windows`` in float64: (frame_p (batch,2), mean2 (n,2)); an empty range gives 0.5."""
    p = torch.sigmoid(torch.as_tensor(logits).detach().double().cpu().reshape(nets, batch, 2))
    frame_p = p.mean(0)
    mean2 = torch.full((len(ranges), 2), 0.5, dtype=torch.float64)
    for k, (lo, hi) in enumerate(ranges):
        if hi > lo:
            mean2[k] = p[:, lo:hi].reshape(-1, 2).mean(0)
    return frame_p, mean2


def face_crop_preprocess_ref(frames_u8, boxes, size=224, dtype=None):
    """``_lib.face_crop_preprocess`` on the CPU: the INTER_AREA restatement, the reference's normalisation, a cast."""
    from oracle import cpu_ref, cv_area
    fr = frames_u8.cpu().numpy() if torch.is_tensor(frames_u8) else np.asarray(frames_u8)
    boxes = [tuple(int(v) for v in b) for b in boxes]
    if not boxes:
        return torch.empty((0, 3, size, size), dtype=dtype or torch.float32)
    return cpu_ref.preprocess_frame(cv_area.face_crops(fr, boxes, size)).to(dtype or torch.float32)


def boxes_all_regimes(nf, H, W):
    """(frame, top, right, bottom, left) rows covering every branch of cv::resize(INTER_AREA) and the frame borders: the
    thirteen boxes of tests/test_parity_gpu.py (a copy)."""
    return [
        (0, 0, 448, 448, 0),                 # 2x2 whole factor: (a+b+c+d+2)>>2
        (1, 10, 672 + 5, 672 + 10, 5),       # 3x3 whole factor: cvRound(sum / 9)
        (2, 0, 448, 672, 0),                 # 3 (y) x 2 (x)
        (0, 100, 324, 324, 100),             # scale 1: copy
        (1, 33, 47 + 310, 33 + 300, 47),     # general shrink, both axes
        (2, 200, 1000, 200 + 511, 603),      # general shrink, factor > 2 on y
        (3, H - 233, W, H, W - 225),         # barely shrinking, touching the bottom-right corner
        (0, 50, 170, 150, 50),               # both axes grow (100 x 120)
        (1, 5, 405, 155, 5),                 # y grows, x shrinks -> bilinear path for both
        (2, 300, 390, 700, 300),             # x grows, y shrinks
        (3, 7, 8, 8, 7),                     # a single pixel
        (3, 0, 223, 225, 0),                 # 225 x 223: one axis either side of 224
        (nf - 1, 0, W, H, 0),                # the whole frame
    ]


def frames_all_regimes():
    """The 4 x 720 x 1280 frames of that test: three of noise, the fourth smooth (ties in the rounding)."""
    nf, H, W = 4, 720, 1280
    rng = np.random.default_rng(5)
    frames = rng.integers(0, 256, (nf, H, W, 3), dtype=np.uint8)
    yy, xx = np.mgrid[0:H, 0:W]
    frames[3] = np.stack([(yy * 3 + xx) % 256, (xx * 2) % 256, (yy * xx // 97) % 256], -1).astype(np.uint8)
    return frames


def fuzz_boxes():
    """The 64-box fuzz of that file: (3 x 480 x 640 frames, boxes from 2 px to the whole frame, any aspect ratio)."""
    nf, H, W = 3, 480, 640
    rng = np.random.default_rng(11)
    frames = rng.integers(0, 256, (nf, H, W, 3), dtype=np.uint8)
    boxes = []
    for _ in range(64):
        h = int(rng.integers(2, H + 1)) if rng.random() < 0.7 else int(rng.choice([112, 224, 448]))
        w = int(rng.integers(2, W + 1)) if rng.random() < 0.7 else int(rng.choice([112, 224, 448]))
        top, left = int(rng.integers(0, H - h + 1)), int(rng.integers(0, W - w + 1))
        boxes.append((int(rng.integers(0, nf)), top, left + w, top + h, left))
    return frames, boxes
