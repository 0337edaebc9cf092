"""Would tests/test_transitions_gpu.py notice a ``gcv_frame_cells``, ``gcv_blend_fit`` or ``gcv_hist_diff_lag`` that is subtly
wrong?  Answered without a GPU, as tests/test_extend_sensitivity_cpu.py does for its kernel: the GPU test compares bit for
bit against the restatements of tests/transutil.py on its videos, so a defect is caught exactly when a restatement WITH
that defect differs from the right one somewhere on those inputs.  A defect that stops differing is fixed by the inputs,
never by dropping it."""
import numpy as np
import pytest

from tests import cutsutil as cu
from tests import transutil as tu

GRIDS = (8, 16, 32)


def _cell_cases():
    """name -> (frames, grid): every frame_cells launch of the GPU test's comparisons"""
    cases = {}
    video, noise = tu.transition_video(), cu.noise_video()
    for g in GRIDS:
        cases[f"transition G{g}"] = (video[:15], g)
        cases[f"noise G{g}"], cases[f"noise[1:] G{g}"], cases[f"noise[3:] G{g}"] = (noise, g), (noise[1:], g), (noise[3:], g)
    cases["tiny G32"], cases["many G16"] = (tu.tiny_video(), 32), (cu.many_video(), 16)
    cases["wide G8"], cases["wide G32"] = (tu.wide_video(), 8), (tu.wide_video(), 32)
    cases["flat G8"], cases["tall G8"], cases["tall[1:] G8"] = (tu.flat_video(), 8), (tu.tall_video(), 8), (tu.tall_video()[1:], 8)
    return cases


def _fit_cases():
    """name -> (cells, lag): every blend_fit launch of the GPU test's comparisons"""
    cases = {}
    video = tu.transition_video()
    for g in GRIDS:
        cells = tu.frame_cells_ref(video, g)
        for lag in (2, 4, 8, 32):
            cases[f"transition G{g} lag {lag}"] = (cells, lag)
        for lag in (2, 3, 5):
            cases[f"extreme G{g} lag {lag}"] = (tu.extreme_cells(g), lag)
    return cases


def _lag_cases():
    """name -> (hist, lag): every hist_diff_lag launch of the GPU test's comparisons"""
    shots = cu.three_shot_video()
    return {f"three shots R{r} lag {lag}": (cu.frame_hist_ref(shots, r), lag) for r in (1, 4) for lag in (1, 4, 8, 14)}


@pytest.fixture(scope="module")
def cell_cases():
    return {name: (*c, tu.frame_cells_ref(*c)) for name, c in _cell_cases().items()}


@pytest.fixture(scope="module")
def fit_cases():
    return {name: (*c, tu.blend_fit_ref(*c)) for name, c in _fit_cases().items()}


@pytest.fixture(scope="module")
def lag_cases():
    return {name: (*c, tu.hist_diff_lag_ref(*c)) for name, c in _lag_cases().items()}


EVERY_FIT = {f"{v} G{g} lag {lag}" for g in GRIDS for v, lags in (("transition", (2, 4, 8, 32)), ("extreme", (2, 3, 5)))
             for lag in lags}
EXTREME = {n for n in EVERY_FIT if n.startswith("extreme")}
SPLIT = {"flat G8", "tall G8", "tall[1:] G8"}
CELL_MUST = {                                                # the cases that have to catch each defect
    "luma without rounding": {"transition G8", "transition G32", "noise G16", "tiny G32", "many G16", "wide G8", "tall G8"},
    "a group's whole sum given to its first pixel's cell": {"transition G8", "transition G32", "noise G8", "noise[1:] G16",
                                                            "tiny G32", "many G16", "wide G8", "wide G32", "tall G8"},
    "at most one edge crossed per group": {"noise G32", "noise[1:] G32", "noise[3:] G32", "tiny G32"},
    "the cell index taken from x G / W": {"transition G8", "transition G16", "transition G32", "noise G16", "noise G32",
                                          "many G16", "wide G32"},
    "column edges rounded": {"transition G8", "transition G16", "transition G32", "noise G8", "noise G32", "many G16",
                             "wide G8", "wide G32", "tall G8"},
    "cells transposed": {"transition G8", "transition G32", "noise G16", "tiny G32", "many G16", "wide G8", "tall G8"},
    "the slice-boundary row counted twice": SPLIT,
    "the slice-boundary row dropped": SPLIT,
}
FIT_MUST = {
    "D taken at lag - 1": EVERY_FIT,
    "m relative to B": EVERY_FIT,
    "the Smd / Smm columns shifted by one k": EVERY_FIT,
    "cells j >= 1 of a thread dropped": {n for n in EVERY_FIT if " G32 " in n},
    "one wave's partial dropped": {n for n in EVERY_FIT if " G8 " not in n},
    "products accumulated in float64": EXTREME,
    "products in 32 bits": EXTREME,
}
LAG_MUST = {
    # no frame of the three shots reaches Y >= 252; it is the same kernel at every lag, and tests/test_cuts_sensitivity_cpu.py
    # pins this defect to cutsutil.ends_pair at lag 1
    "bin 63 left out of the distance": set(),
    "a - b without the absolute value": {f"three shots R{r} lag {lag}" for r in (1, 4) for lag in (1, 4, 8, 14)},
    "the second frame lag regions on": {f"three shots R4 lag {lag}" for lag in (1, 4, 8, 14)},
    "lag ignored": {f"three shots R{r} lag {lag}" for r in (1, 4) for lag in (4, 8, 14)},
}


def test_every_defect_is_audited():
    assert set(CELL_MUST) == set(tu.CELL_DEFECTS) and len(tu.CELL_DEFECTS) == 8
    assert set(FIT_MUST) == set(tu.FIT_DEFECTS) and len(tu.FIT_DEFECTS) == 7
    assert set(LAG_MUST) == set(cu.DIFF_DEFECTS) and len(cu.DIFF_DEFECTS) == 4


def _audit(cases, alt, defect, must):
    caught = {name for name, (*args, right) in cases.items() if not np.array_equal(alt(*args, defect=defect), right)}
    print(f"\n{defect}: caught by {sorted(caught)}")
    assert must <= caught, must - caught


@pytest.mark.parametrize("defect", tu.CELL_DEFECTS)
def test_a_frame_cells_defect_changes_the_gpu_tests_cells(cell_cases, defect):
    _audit(cell_cases, tu.frame_cells_alt, defect, CELL_MUST[defect])


@pytest.mark.parametrize("defect", tu.FIT_DEFECTS)
def test_a_blend_fit_defect_changes_the_gpu_tests_sums(fit_cases, defect):
    _audit(fit_cases, tu.blend_fit_alt, defect, FIT_MUST[defect])


@pytest.mark.parametrize("defect", cu.DIFF_DEFECTS)
def test_a_hist_diff_lag_defect_changes_the_gpu_tests_distances(lag_cases, defect):
    _audit(lag_cases, cu.hist_diff_alt, defect, LAG_MUST[defect])


def test_without_a_defect_nothing_differs(cell_cases, fit_cases, lag_cases):
    for cases, alt in ((cell_cases, tu.frame_cells_alt), (fit_cases, tu.blend_fit_alt), (lag_cases, cu.hist_diff_alt)):
        for name, (*args, right) in cases.items():
            assert np.array_equal(alt(*args), right), name


def test_the_inputs_hold_what_the_gpu_test_says(cell_cases, fit_cases):
    S = {name: tu.cells_slices(c[0].shape[0], c[0].shape[1], c[1]) for name, c in cell_cases.items()}
    assert {name for name, s in S.items() if s > 1} == SPLIT and S["flat G8"] == 8 and S["tall G8"] == S["tall[1:] G8"] == 2
    frames = cell_cases["transition G32"][0]
    assert frames.shape == (15, 90, 130, 3) and 390 % 4
    assert {b - a for a, b in zip(cu.edges(90, 32), cu.edges(90, 32)[1:])} == {2, 3}
    assert {b - a for a, b in zip(cu.edges(130, 32), cu.edges(130, 32)[1:])} == {4, 5}          # a group crosses cell edges
    assert {b - a for a, b in zip(cu.edges(53, 32), cu.edges(53, 32)[1:])} == {1, 2}            # a group holds two whole cells
    assert cell_cases["noise G8"][0].shape == (4, 37, 53, 3) and (37 * 53 * 3) % 2 == 1
    assert (cell_cases["tiny G32"][2] == cu.luma(tu.tiny_video()).reshape(2, -1)).all()
    assert cell_cases["many G16"][0].shape[0] * 16 == 1120 >= cu.FH_TARGET_WGS
    assert (1103 + 3) // 4 == 276 > 256 and cell_cases["wide G8"][0].shape == (1, 37, 1103, 3)
    assert (cell_cases["flat G8"][2] == 255 * 4096).all()
    assert {b - a for a, b in zip(cu.edges(161, 8), cu.edges(161, 8)[1:])} == {20, 21}
    for g in GRIDS:
        cells = tu.extreme_cells(g)
        assert all(sum(int(v) ** 2 for v in row) < 2 ** 62 for row in cells)                     # the header's bound for a row
        for lag in (2, 3, 5):
            assert int(fit_cases[f"extreme G{g} lag {lag}"][2].max()) > 2 ** 62                  # beyond float64's 2^53
