"""Would tests/test_quality_gpu.py notice a ``gcv_face_quality`` that is subtly wrong?  Answered without a GPU, as
tests/test_extend_sensitivity_cpu.py does for its kernel: the GPU test compares bit for bit against
``qualityutil.face_quality_ref`` on the inputs of tests/qualityutil.py, so a defect is caught exactly when a restatement
WITH that defect differs from the right one somewhere on those inputs.  A defect that stops differing is fixed by the
inputs, never by dropping it."""
import numpy as np
import pytest

from tests import qualityutil as qu

GRIDS = (16, 32, 64)


def _cases():
    """name -> (frames, boxes, grid): every comparison of the GPU test"""
    cases = {}
    for g in (16, 32):
        cases[f"random {g}"] = (*qu.fuzz_boxes(g), g)
    for g in GRIDS:
        cases[f"edge {g}"] = (qu.fuzz_boxes(16)[0], qu.edge_boxes(g), g)
        cases[f"flat {g}"] = (*qu.flat_case(), g)
        cases[f"checkerboard {g}"] = (*qu.checkerboard(g, 2), g)
    frames, boxes = qu.unaligned_case()
    cases["unaligned 16"] = (frames[1:], boxes, 16)
    cases["largest 64"] = (*qu.largest_case(), 64)
    return cases


@pytest.fixture(scope="module")
def cases():
    return {name: (*c, qu.face_quality_ref(*c)) for name, c in _cases().items()}


EDGES = {"edge 16", "edge 32", "edge 64"}
BOARDS = {"checkerboard 16", "checkerboard 32", "checkerboard 64"}
NOISE = {"random 16", "random 32", "unaligned 16", "largest 64"} | EDGES
MUST = {                                                     # the cases that have to catch each defect
    "luma without rounding": NOISE | {"flat 16", "flat 32", "flat 64"},
    "cell mean floored": NOISE,
    "row edges from w, column edges from h": NOISE,
    "dark <= 16": {"random 32", "edge 32", "edge 64", "largest 64"},
    "bright >= 239": {"random 32", "edge 32", "edge 64", "largest 64"},
    "GX wraps at the last column": NOISE,
    "GY wraps at the last row": NOISE | BOARDS,
    "the Laplacian over border cells, neighbours clamped": NOISE | BOARDS,
    "GX / GY swapped": NOISE,
    "cells of the later 256-cell trips dropped": {"random 32", "edge 32", "edge 64", "flat 32", "flat 64", "checkerboard 32",
                                                  "checkerboard 64", "largest 64"},
    "one wave's partial dropped": NOISE | BOARDS | {"flat 16", "flat 32", "flat 64"},
    "totals in signed 32 bits": {"checkerboard 64"},
    "S2 in 24 bits": {"random 32", "edge 32", "edge 64", "flat 32", "flat 64", "checkerboard 32", "checkerboard 64", "largest 64"},
}


def test_every_defect_is_audited():
    assert set(MUST) == set(qu.DEFECTS) and len(qu.DEFECTS) == 13


@pytest.mark.parametrize("defect", qu.DEFECTS)
def test_a_defect_changes_the_gpu_tests_rows(cases, defect):
    caught = {name for name, (frames, boxes, grid, right) in cases.items()
              if not np.array_equal(qu.face_quality_alt(frames, boxes, grid, defect=defect), right)}
    print(f"\n{defect}: caught by {sorted(caught)}")
    assert MUST[defect] <= caught, MUST[defect] - caught


def test_without_a_defect_nothing_differs(cases):
    for name, (frames, boxes, grid, right) in cases.items():
        assert np.array_equal(qu.face_quality_alt(frames, boxes, grid), right), name


def test_the_inputs_hold_what_the_gpu_test_says(cases):
    for g in (16, 32):
        boxes = cases[f"random {g}"][1]
        assert len(boxes) == 48 and {0} == {min(b[1] for b in boxes), min(b[4] for b in boxes)}
        assert max(b[3] for b in boxes) == 120 and max(b[2] for b in boxes) == 160
    for g in GRIDS:
        boxes = cases[f"edge {g}"][1]
        assert [(b[3] - b[1], b[2] - b[4]) for b in boxes[:3]] == [(g, g + 1), (g + 1, g), (g, g)]
        assert boxes[3][1:] == (0, 160, 120, 0) and len(boxes) == 13
        n = g * g
        assert cases[f"flat {g}"][3][:3].tolist() == [[g, n * 124, n * 124 * 124, 0, 0, 0, 0, 0], [g, 0, 0, 0, 0, 0, n, 0],
                                                      [g, n * 255, n * 255 * 255, 0, 0, 0, 0, n]]
        # the checkerboard: every interior Laplacian is +-1020, the kernel's |l| <= 1020, and every difference +-255
        row = cases[f"checkerboard {g}"][3][0].tolist()
        assert row == [g, n // 2 * 255, n // 2 * 255 ** 2, (g - 2) ** 2 * 1020 ** 2, g * (g - 1) * 255 ** 2, g * (g - 1) * 255 ** 2,
                       n // 2, n // 2]
    assert cases["checkerboard 64"][3][0].tolist() == qu.CHECKERBOARD_64 and 2 ** 31 < qu.CHECKERBOARD_64[3] < 2 ** 32
    assert 16 * 1020 ** 2 < 2 ** 24 and 64 * 16 * 1020 ** 2 < 2 ** 31                # a lane's and a wave's sum, as the kernel states
    # without the checkerboard nothing comes near 2^31
    assert max(int(c[3][:, 1:].max()) for name, c in cases.items() if name not in BOARDS) < 2 ** 29
    assert cases["unaligned 16"][0].shape == (3, 37, 53, 3) and (37 * 53 * 3) % 2 == 1
    assert cases["largest 64"][0].shape == (2, 300, 400, 3) and cases["largest 64"][1][0] == (0, 0, 400, 300, 0)
