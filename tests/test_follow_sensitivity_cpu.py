"""Would tests/test_follow_gpu.py notice a ``gcv_track_match`` that is subtly wrong?  Answered without a GPU, as
tests/test_extend_sensitivity_cpu.py does for ``gcv_track_chain``: the GPU test compares bit for bit against
``followutil.track_match_ref`` on the cases of tests/followutil.py, so a defect is caught exactly when a restatement WITH
that defect differs from the right one somewhere on those inputs.  Each defect below is one a kernel with these three
phases could plausibly have; a defect that stops differing is fixed by the inputs, never by dropping it."""
import numpy as np
import pytest

from tests import followutil as fu


def _cases():
    """name -> (frames, jobs, grid, radius): what the GPU test launches (of the random jobs radius 5 and 8, the one with 289
    candidates: the four validity defects each show on a handful of rows at one radius and not at the other; of the
    largest configuration, radius 16)"""
    frames, jobs, _ = fu.path_case()
    cases = {"path": (frames, jobs, 16, 4)}
    for grid in (16, 32):
        for radius in (5, 8):
            cases[f"random {grid} r{radius}"] = (*fu.fuzz_case(lo=grid), grid, radius)
    cases["largest"] = (*fu.largest_case(), 64, 16)
    for grid, k, radius in fu.TIE_CASES:
        cases[f"tie {grid} {k} {radius}"] = (*fu.tie_case(grid, k), grid, radius)
    for grid, k in ((16, 3), (32, 2)):
        cases[f"far tie {grid}"] = (*fu.far_tie_case(grid, k), grid, 8)
        cases[f"wave tie {grid}"] = (*fu.far_tie_case(grid, k, 6, 6), grid, 8)
    cases["bound"] = fu.bound_case()
    return cases


@pytest.fixture(scope="module")
def cases():
    return {name: (*c, fu.track_match_ref(*c)) for name, c in _cases().items()}


RANDOM = {"random 16 r5", "random 16 r8", "random 32 r5", "random 32 r8"}
TIES = {"tie 16 3 4", "tie 16 3 8", "tie 32 2 8"}
FAR = {"far tie 16", "far tie 32"}
MUST = {                                                     # the cases that have to catch each defect
    "luma without rounding": {"path", "largest"} | RANDOM,
    "cell mean floored": {"path", "largest"} | RANDOM | TIES,
    "edges truncated toward zero": {"path", "largest"} | RANDOM,
    "validity: top off by one": RANDOM,
    "validity: bottom off by one": RANDOM,
    "validity: left off by one": {"random 32 r5", "random 32 r8"},
    "validity: right off by one": {"random 32 r5"},
    "window from template a's frame": {"path", "largest", "bound"} | RANDOM,
    "template b built with a's edges": {"largest"} | RANDOM,
    "templates swapped": {"largest"} | RANDOM,
    "cost0 equal to the best cost": {"path", "largest"} | RANDOM | TIES | FAR,
    "oy / ox in cells": {"path", "largest"} | RANDOM | TIES | FAR,
    "ox scaled by h": {"path", "largest"} | RANDOM,
    "tie-break: d2 dropped": TIES,
    "tie-break: dx before dy": TIES | FAR,
    "tie-break: the last equal candidate wins": TIES | FAR,
    "the last candidate is never evaluated": RANDOM,
    "candidates of the second loop trip dropped": {"largest"} | FAR,
    "one wave's minimum ignored": {"largest", "random 32 r8", "wave tie 16", "wave tie 32"},
    "template sums in 16 bits": {"largest", "random 32 r5", "random 32 r8", "bound"},
    "the key keeps 29 bits of cost": {"bound"},
}


def test_every_defect_is_audited():
    assert set(MUST) == set(fu.DEFECTS) and len(fu.DEFECTS) == 21


@pytest.mark.parametrize("defect", fu.DEFECTS)
def test_a_defect_changes_the_gpu_tests_rows(cases, defect):
    caught = set()
    for name, (frames, jobs, grid, radius, right) in cases.items():
        if not np.array_equal(fu.track_match_alt(frames, jobs, grid, radius, defect=defect), right):
            caught.add(name)
    print(f"\n{defect}: caught by {sorted(caught)}")
    assert MUST[defect] <= caught, MUST[defect] - caught


def test_without_a_defect_nothing_differs(cases):
    for name, (frames, jobs, grid, radius, right) in cases.items():
        assert np.array_equal(fu.track_match_alt(frames, jobs, grid, radius), right), name


def test_the_inputs_hold_what_the_gpu_test_says(cases):
    frames, jobs, grid, radius, right = cases["path"]
    assert [(p[0] + int(o[0]), p[1] + int(o[1])) for p, o in zip(fu.path_case()[2], right)] == fu.PATH_FOLLOWED
    for grid in (16, 32):
        frames, jobs, _, _, right = cases[f"random {grid} r8"]
        sides = [(j[c + 3] - j[c + 1], j[c + 2] - j[c + 4]) for j in jobs for c in (0, 5, 11)]
        assert len(jobs) == 48 and all(grid <= s <= 100 and s % 16 for hw in sides for s in hw)
        assert any(j[10] == 0 for j in jobs) and any(j[16] == 0 for j in jobs)
        assert {0} == {min(j[1] for j in jobs), min(j[4] for j in jobs)}
        assert max(j[3] for j in jobs) == 120 and max(j[2] for j in jobs) == 160
    # the path, the random jobs and the largest configuration hold no cost tie that decides a row: the key's tie-break is
    # decided by the tie cases alone
    for name in ("path", "largest", *sorted(RANDOM)):
        frames, jobs, grid, radius, right = cases[name]
        for defect in fu.DEFECTS[13:16]:
            assert defect.startswith("tie-break") and \
                np.array_equal(fu.track_match_alt(frames, jobs, grid, radius, defect=defect), right), (name, defect)
    frames, jobs, grid, radius, right = cases["largest"]
    assert grid == 64 and len(jobs) == 12 and frames.shape == (3, 256, 256, 3)
    for key, rows in fu.TIE_ROWS.items():
        frames, jobs, grid, radius, right = cases["tie %d %d %d" % key]
        assert right.tolist() == rows and (frames[0] == frames[1]).all() and (frames[..., 0] == frames[..., 2]).all()
        assert (frames[0, 1:, :-1] == frames[0, :-1, 1:]).all()                     # constant along the anti-diagonals
    for name in FAR:
        frames, jobs, grid, radius, right = cases[name]
        j = jobs[0]
        h, w = j[3] - j[1], j[2] - j[4]
        assert radius == 8 and j[1] - h // 2 >= 0 and j[4] - w // 2 >= 0 and j[3] + h // 2 <= 160 and j[2] + w // 2 <= 160
        assert right[0, :3].tolist() == [7 * h // grid, 8 * w // grid, 0] and 15 * 17 + 16 >= 256      # all 289 are valid
    for name in ("wave tie 16", "wave tie 32"):
        frames, jobs, grid, radius, right = cases[name]
        side = jobs[0][3] - jobs[0][1]
        assert right[0, :3].tolist() == [6 * side // grid, 6 * side // grid, 0] and 192 <= (6 + 8) * 17 + 6 + 8 < 256
    frames, jobs, grid, radius, right = cases["bound"]
    assert grid == 64 and all(j[10] + j[16] == 1024 for j in jobs) and any(j[16] == 0 for j in jobs)
    assert right.tolist() == [[0, 0, fu.COST_BOUND, fu.COST_BOUND]] * 3 and 2 ** 29 < fu.COST_BOUND < 2 ** 31
