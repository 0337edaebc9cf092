"""CPU restatement, in numpy, of the arithmetic of gcv_scan_annotate (include/genconvit_hip.h; csrc/annotate.hip), written
from the header's statement: outlines, number tabs, the timeline strip and its cursor, all in integers, so the kernel is
expected to be bit-equal to this (tests/test_annotate_gpu.py).  Vectorised per mark (slices and index grids).  Also the same
with one planted defect (tests/test_annotate_sensitivity_cpu.py) and the cases the CPU and GPU tests share.  Test
infrastructure: the product does not import it."""
import numpy as np
import torch

FONT = ("111101101101111", "010110010010111", "111001111100111", "111001111001111", "101101111001001",
        "111100111001111", "111100111101111", "111001001001001", "111101111101111", "111101111001111")

DEFECTS = ("far edges off by one", "digits least significant first", "the tab is not clipped to its box",
           "marks in reverse order", "the timeline under the marks", "a cursor always one column wide",
           "the lane taken from H", "t rounded", "ink threshold with >", "frame_no ignored")


def rgb(colour):
    colour = int(colour) & 0xFFFFFF
    return colour & 255, colour >> 8 & 255, colour >> 16


def pack(r, g, b):
    return int(r) | int(g) << 8 | int(b) << 16


def tab_cells(digits):
    """The (7, 4 nd + 1) cells of a tab, True where there is ink."""
    cells = np.zeros((7, 4 * len(digits) + 1), dtype=bool)
    for k, d in enumerate(digits):
        for i, c in enumerate(FONT[d]):
            cells[1 + i // 3, 1 + 4 * k + i % 3] = c == "1"
    return cells


def _as_numpy(frames):
    return frames.detach().cpu().numpy() if torch.is_tensor(frames) else np.asarray(frames)


def annotate_alt(frames, frame_no, marks, timeline=None, strip=0, defect=None):
    """gcv_scan_annotate on the CPU, with one of ``DEFECTS`` planted (None: the header's arithmetic): a uint8 (F,H,W,3)
    tensor, a copy of ``frames`` with the marks drawn in row order and the timeline over them."""
    assert defect is None or defect in DEFECTS, defect
    out = np.array(_as_numpy(frames), dtype=np.uint8, copy=True)
    nf, H, W, _ = out.shape
    marks = np.asarray(_as_numpy(marks) if torch.is_tensor(marks) else marks, dtype=np.int64).reshape(-1, 8)
    frame_no = [int(v) for v in (_as_numpy(frame_no) if torch.is_tensor(frame_no) else frame_no)]

    def draw_timeline():
        if strip <= 0 or nf == 0:
            return
        tl = np.asarray(_as_numpy(timeline), dtype=np.int64) & 0xFFFFFF
        lanes, T = tl.shape
        assert 1 <= lanes <= 8 and lanes <= strip <= H and T >= 1 and T * W < 1 << 31
        ys = H - strip
        yy = np.arange(ys, H, dtype=np.int64)
        lane = ((yy - ys) * lanes) // (H if defect == "the lane taken from H" else strip)
        xx = np.arange(W, dtype=np.int64)
        t = np.minimum((xx * T + W // 2) // W, T - 1) if defect == "t rounded" else (xx * T) // W
        band = tl[lane][:, t]
        band = np.stack((band & 255, band >> 8 & 255, band >> 16), axis=-1).astype(np.uint8)
        for f in range(nf):
            out[f, ys:] = band
            c = f if defect == "frame_no ignored" else frame_no[f]
            if 0 <= c < T:
                x0 = (c * W) // T
                x1 = x0 + 1 if defect == "a cursor always one column wide" else max(x0 + 1, ((c + 1) * W) // T)
                out[f, ys:, x0:x1] = 255

    if defect == "the timeline under the marks":
        draw_timeline()
    for f, top, right, bottom, left, colour, thick, label in (marks[::-1] if defect == "marks in reverse order" else marks).tolist():
        if not (0 <= f < nf and 0 <= top < bottom <= H and 0 <= left < right <= W and 1 <= thick <= 16 and -1 <= label <= 999):
            continue
        col = rgb(colour)
        box = out[f, top:bottom, left:right]
        dy = np.arange(bottom - top)[:, None]
        dx = np.arange(right - left)[None, :]
        off = 1 if defect == "far edges off by one" else 0              # bottom - y instead of bottom - 1 - y
        edge = (dy < thick) | (bottom - top - 1 - dy + off < thick) | (dx < thick) | (right - left - 1 - dx + off < thick)
        box[edge] = col
        if label < 0:
            continue
        digits = [int(c) for c in str(label)]
        if defect == "digits least significant first":
            digits = digits[::-1]
        ink = np.kron(tab_cells(digits), np.ones((thick, thick), dtype=bool))      # cy = (y - top) / thick, cx alike
        luma = (77 * col[0] + 150 * col[1] + 29 * col[2]) >> 8
        dark = luma > 128 if defect == "ink threshold with >" else luma >= 128
        if defect == "the tab is not clipped to its box":
            box = out[f, top:, left:]
        th, tw = min(ink.shape[0], box.shape[0]), min(ink.shape[1], box.shape[1])
        box[:th, :tw] = np.where(ink[:th, :tw, None], np.uint8(0 if dark else 255), np.array(col, dtype=np.uint8))
    if defect != "the timeline under the marks":
        draw_timeline()
    return torch.from_numpy(out)


def annotate_ref(frames, frame_no, marks, timeline=None, strip=0):
    """gcv_scan_annotate on the CPU."""
    return annotate_alt(frames, frame_no, marks, timeline, strip)


# ----------------------------------------------------------------------------- shared inputs
def frames_of(shape, seed):
    return torch.randint(0, 256, shape, dtype=torch.uint8, generator=torch.Generator().manual_seed(seed))


def timeline_of(lanes, T, seed):
    """(lanes, T) int64 of packed colours with a set top byte, which the entry ignores; no two neighbours alike"""
    g = torch.Generator().manual_seed(seed)
    tl = torch.randint(0, 1 << 24, (lanes, T), dtype=torch.int64, generator=g)
    tl = (tl & ~0xFF) | ((torch.arange(T)[None, :] * 37 + torch.arange(lanes)[:, None] * 101) & 0xFF)    # r differs
    return tl | (0x5A << 24)


LABELS = (-1, 0, 9, 10, 99, 100, 999, 40, 123, 7)


def random_marks(nf, H, W, n, seed, max_side=None, thicks=(1, 1, 2, 3, 5, 16)):
    """n marks with boxes from 1 pixel to ``max_side`` (default: the frame) a side, every kind of label, both ink colours"""
    g = torch.Generator().manual_seed(seed)
    r = lambda lo, hi: int(torch.randint(lo, hi + 1, (1,), generator=g))
    marks = []
    for i in range(n):
        h, w = r(1, min(H, max_side or H)), r(1, min(W, max_side or W))
        top, left = r(0, H - h), r(0, W - w)
        marks.append((r(0, nf - 1), top, left + w, top + h, left, r(0, (1 << 24) - 1), thicks[r(0, len(thicks) - 1)],
                      LABELS[i % len(LABELS)]))
    return marks


GREY128, GREY127 = pack(128, 128, 128), pack(127, 127, 127)          # luma exactly 128 (black ink) and 127 (white ink)


def label_marks(f=0):
    """Every label length on boxes that hold the tab and boxes that clip it, both ink colours and the luma boundary;
    needs frames of at least 60 x 120."""
    marks = []
    for i, (label, colour) in enumerate(zip((-1, 0, 9, 10, 99, 100, 999), (0x00FF00, 0x0000A0, GREY128, GREY127, 0xFFFFFF,
                                                                           0x000000, 0x00D7FF))):
        marks.append((f, 2, 16 * i + 15, 12, 16 * i + 1, colour, 1, label))                # 10 x 14: holds a 7 x 13 tab
    marks += [(f, 14, 40, 30, 10, 0x00FF00, 2, 40),                                          # the 16 x 30 box of the CPU test
              (f, 14, 50, 19, 44, GREY128, 2, 123), (f, 14, 56, 17, 52, GREY127, 1, 999),    # smaller than their tabs
              (f, 32, 118, 59, 60, 0x3030F0, 3, 407), (f, 32, 58, 40, 2, 0xF0F030, 2, 85),
              (f, 42, 23, 43, 22, 0x123456, 1, 5), (f, 44, 70, 59, 3, 0x808080, 16, 68)]     # 1 x 1; thick 16: one cell, over the 407
    return marks


RAW = "rows that draw nothing"                # the case that goes through the C entry: _lib.scan_annotate refuses its rows


def cases(full_hd=False):
    """name -> (frames, frame_no, marks, timeline, strip): what tests/test_annotate_gpu.py launches and
    tests/test_annotate_sensitivity_cpu.py audits."""
    c = {}
    # tiny frames, several in one block: marks of every kind, on every frame and on none (frame 3 has none)
    marks = [m for m in random_marks(5, 37, 53, 40, 1) if m[0] != 3]
    c["tiny frames"] = (frames_of((5, 37, 53, 3), 2), [3, 0, 9, 4, 7], marks, timeline_of(2, 10, 3), 4)
    # the same with rows the binding refuses and the entry itself skips, one of each kind, among the others
    junk = [(7, 0, 5, 5, 0, 0xFFFFFF, 1, 1), (-1, 0, 5, 5, 0, 0xFFFFFF, 1, 1), (0, 5, 60, 9, 2, 0xFFFFFF, 1, 1),
            (0, 30, 9, 38, 2, 0xFFFFFF, 1, 1), (1, 5, 9, 5, 2, 0xFFFFFF, 1, 1), (1, 5, 2, 9, 2, 0xFFFFFF, 1, 1),
            (1, -1, 9, 9, 2, 0xFFFFFF, 1, 1), (1, 5, 9, 9, -2, 0xFFFFFF, 1, 1), (1, 5, 9, 9, 2, 0xFFFFFF, 0, 1),
            (1, 5, 9, 9, 2, 0xFFFFFF, 17, 1), (1, 5, 9, 9, 2, 0xFFFFFF, 1, 1000), (1, 5, 9, 9, 2, 0xFFFFFF, 1, -2)]
    c[RAW] = (c["tiny frames"][0], [3, 0, 9, 4, 7], [m for pair in zip(junk, marks) for m in pair] + marks[len(junk):],
              timeline_of(2, 10, 3), 4)
    for W in (1, 2, 3, 5, 641, 1024):
        c[f"width {W}"] = (frames_of((3, 9, W, 3), 10 + W), [2, 0, 1], random_marks(3, 9, W, 6, 20 + W), timeline_of(2, 3, 30 + W), 3)
    c["many marks"] = (frames_of((2, 130, 250, 3), 40), [0, 1], random_marks(2, 130, 250, 300, 41, max_side=12), None, 0)
    c["overlapping"] = (frames_of((1, 60, 90, 3), 50), [0],
                        [(0, 5, 70, 50, 10, 0xFF0000, 3, 12), (0, 20, 85, 55, 40, 0x00FF00, 2, 345),
                         (0, 22, 60, 40, 44, 0x0000FF, 3, 6), (0, 5, 70, 50, 10, 0x00FFFF, 1, -1),
                         (0, 0, 90, 60, 0, 0xFF00FF, 2, 0)], timeline_of(1, 1, 51), 2)
    c["outline edges"] = (frames_of((1, 40, 40, 3), 60), [0],
                          [(0, 3, 4, 4, 3, 0x112233, 1, -1), (0, 3, 8, 4, 7, 0x112233, 1, 3),                # 1 x 1
                           (0, 10, 30, 30, 10, 0x445566, 16, -1), (0, 31, 39, 39, 31, 0x778899, 4, -1),    # 2 thick >= side
                           (0, 0, 40, 9, 31, 0x99AABB, 3, -1), (0, 5, 7, 12, 0, 0xCCDDEE, 2, -1)], None, 0)
    c["labels"] = (frames_of((2, 60, 120, 3), 70), [0, 1], label_marks(0) + label_marks(1)[::2], None, 0)
    W, H = 53, 20
    for T in (1, 5, W, 4 * W + 3):
        c[f"timeline T {T}"] = (frames_of((4, H, W, 3), 80 + T), [-1, T - 1, T, T // 2],
                                [(1, 8, 30, 20, 10, 0xABCDEF, 2, 40)], timeline_of(2, T, 81 + T), 7)
    for lanes in (1, 2, 3, 8):
        for strip in sorted({lanes, 7, H} - set(range(lanes))):
            c[f"timeline lanes {lanes} strip {strip}"] = (frames_of((2, H, W, 3), 90 + lanes), [4, 1],
                                                          [(0, 2, 50, 18, 30, 0x13579B, 1, 8)], timeline_of(lanes, 5, 91 + strip), strip)
    c["timeline strip 0"] = (frames_of((2, H, W, 3), 95), [4, 1], [(0, 2, 50, 18, 30, 0x13579B, 1, 8)], timeline_of(2, 5, 96), 0)
    c["frame_no"] = (frames_of((3, H, W, 3), 97), [7, 3, 5], [], timeline_of(2, 10, 98), 5)
    if full_hd:
        c["full hd"] = (frames_of((4, 1080, 1920, 3), 100), [0, 1, 2, 3],
                        random_marks(4, 1080, 1920, 16, 101, max_side=700, thicks=(4,)), timeline_of(2, 4, 102), 30)
    return c
