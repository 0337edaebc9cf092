"""Would tests/test_extend_gpu.py notice a step loop that is subtly wrong?  Answered without a GPU, as
tests/test_persons_sensitivity_cpu.py does for its kernels: the GPU test compares bit for bit against
``extendutil.track_chain_ref`` on the cases of tests/extendutil.py, so a defect is caught exactly when a restatement WITH
that defect differs from the right one somewhere on those inputs.  Each defect below is one a kernel that walks a chain
could plausibly have; a defect that stops differing is fixed by the inputs, never by dropping it."""
import numpy as np
import pytest

from tests import extendutil as eu


def _cases():
    """name -> (frames, jobs, grid, radius): what the GPU test launches (of the random chains, one radius per grid is
    enough here), including the second launch of the split chains"""
    cases = {"moving": eu.moving_case(), "stop": eu.stop_case(), "border": eu.border_case()}
    for grid in (16, 32):
        cases[f"random {grid}"] = (*eu.random_case(grid), grid, 5)
    for name in ("moving", "border"):
        frames, jobs, grid, radius = cases[name]
        jobs = [j for j in jobs if j[7] >= 3]
        head, _ = eu.split(jobs, 2, [(0, 0)] * len(jobs))
        first = eu.track_chain_ref(frames, head, grid, radius)
        cases[f"{name}, continued"] = (frames, eu.split(jobs, 2, first[:, :, :2].sum(1).tolist())[1], grid, radius)
    return cases


@pytest.fixture(scope="module")
def cases():
    return {name: (*c, eu.track_chain_ref(*c)) for name, c in _cases().items()}


MUST = {                                                     # the cases that have to catch each defect
    "the prior is not advanced": {"moving", "stop", "border", "random 16", "random 32"},
    "dir is ignored": {"moving", "border", "random 16", "random 32"},
    "validity at the template's position": {"moving", "random 16", "random 32"},
    "stop compared with >=": {"stop"},
    "the chain goes on after a stop": {"stop"},
    "cost0 carried over": {"moving", "stop", "border", "random 16", "random 32"},
    "(py, px) ignored": {"moving, continued", "border, continued", "border", "random 16", "random 32"},
    "the tie-break is dropped": {"random 16", "random 32"},
}


def test_every_defect_of_the_issue_is_audited():
    assert set(MUST) == set(eu.DEFECTS) and len(eu.DEFECTS) == 8


@pytest.mark.parametrize("defect", eu.DEFECTS)
def test_a_step_loop_defect_changes_the_gpu_tests_rows(cases, defect):
    caught = set()
    for name, (frames, jobs, grid, radius, right) in cases.items():
        if not np.array_equal(eu.track_chain_alt(frames, jobs, grid, radius, defect=defect), right):
            caught.add(name)
    print(f"\n{defect}: caught by {sorted(caught)}")
    assert MUST[defect] <= caught, MUST[defect] - caught


def test_without_a_defect_nothing_differs(cases):
    for name, (frames, jobs, grid, radius, right) in cases.items():
        assert np.array_equal(eu.track_chain_alt(frames, jobs, grid, radius), right), name


def test_the_inputs_hold_what_the_gpu_test_says(cases):
    frames, jobs, grid, radius, right = cases["moving"]
    assert len(jobs) == 2 and {j[6] for j in jobs} == {1, -1} and all(j[7] == 5 for j in jobs)
    assert all(len({tuple(s[:2]) for s in rows.tolist()}) == 5 for rows in right)        # a new displacement at every step
    assert jobs[0][4] == 0 and (right[0, :3, 1] > 0).all() and (right[0, 3:, 1] < 0).all()   # from the border, and back
    frames, jobs, grid, radius, right = cases["stop"]
    c = right[0, :, 2]
    assert (c >= 0).all() and jobs[1][10] == max(c[0], c[1]) and jobs[2][10] == c[2] - 1 and jobs[3][10] == c[2]
    assert max(c[3], c[4]) < c[2]                                                        # it would match again
    frames, jobs, grid, radius, right = cases["border"]
    t, l, h, w = jobs[0][1], jobs[0][4], jobs[0][3] - jobs[0][1], jobs[0][2] - jobs[0][4]
    room = []
    for oy, ox, _, _ in right[0].tolist():
        room.append((96 - t - h, 128 - l - w))
        t, l = t + oy, l + ox
    assert all(a > b for a, b in zip(room, room[1:])) and room[-1][0] < 8 * h / 16          # fewer candidates every step
    for grid in (16, 32):
        frames, jobs, _, _, right = cases[f"random {grid}"]
        assert len(jobs) == 48 and {j[7] for j in jobs} == {1, 2, 3, 4, 5} and any(j[8] or j[9] for j in jobs)
        assert (frames[2] == frames[2, 0, 0]).all()                                         # the flat frame: ties
    ended = [bool((r[:j[7], 2] < 0).any()) for j, r in zip(cases["random 32"][1], cases["random 32"][4])]
    assert any(ended) and not all(ended)
    frames, jobs, grid, radius = eu.large_case()
    assert (grid, radius) == (64, 32) and all(j[7] == 3 for j in jobs) and frames.shape == (3, 256, 256, 3)
