"""Would tests/test_annotate_gpu.py notice a drawing kernel that is subtly wrong?  Answered without a GPU, as
tests/test_extend_sensitivity_cpu.py does for its kernel: the GPU test compares bit for bit against
``annotateutil.annotate_ref`` on the cases of tests/annotateutil.py, so a defect is caught exactly when a restatement WITH
that defect differs from the right one somewhere on those inputs.  Each defect below is one a kernel that draws boxes,
digits and a strip could plausibly have; a defect that stops differing is fixed by the inputs, never by dropping it."""
import pytest
import torch

from tests import annotateutil as au


@pytest.fixture(scope="module")
def cases():
    return {name: (*c, au.annotate_ref(*c)) for name, c in au.cases().items()}


TIMELINES = {f"timeline T {T}" for T in (1, 5, 53, 215)} | \
            {f"timeline lanes {l} strip {s}" for l, ss in ((1, (1, 7, 20)), (2, (2, 7, 20)), (3, (3, 7, 20)), (8, (8, 20))) for s in ss}

MUST = {                                                     # the cases that have to catch each defect
    "far edges off by one": {"tiny frames", "many marks", "overlapping", "outline edges", "labels", "width 641", "width 1024"},
    "digits least significant first": {"tiny frames", "many marks", "overlapping", "labels", "timeline T 1"},
    "the tab is not clipped to its box": {"tiny frames", "many marks", "overlapping", "outline edges", "labels"},
    "marks in reverse order": {"tiny frames", "many marks", "overlapping", "labels"},
    "the timeline under the marks": {"tiny frames", "overlapping", "timeline T 1", "timeline T 5", "timeline lanes 2 strip 7",
                                     "timeline lanes 1 strip 20"},
    "a cursor always one column wide": {"tiny frames", "timeline T 1", "timeline T 5", "timeline lanes 2 strip 7", "frame_no",
                                        "width 641", "width 1024"},
    "the lane taken from H": {"tiny frames", "timeline T 5", "timeline lanes 2 strip 7", "timeline lanes 3 strip 7",
                              "timeline lanes 8 strip 8", "timeline lanes 3 strip 3", "frame_no", "width 641"},
    "t rounded": {"tiny frames", "timeline T 5", "timeline T 215",            # not T = W: there x T / W is whole
 "timeline lanes 2 strip 7", "frame_no",
                  "width 641", "width 1024", "width 5"},
    "ink threshold with >": {"labels"},
    "frame_no ignored": {"tiny frames", "frame_no", "timeline T 5", "timeline lanes 2 strip 7", "width 641"},
}


def test_every_defect_of_the_issue_is_audited(cases):
    assert set(MUST) == set(au.DEFECTS) and len(au.DEFECTS) == 10
    assert all(names <= set(cases) for names in MUST.values()) and TIMELINES <= set(cases)


@pytest.mark.parametrize("defect", au.DEFECTS)
def test_a_drawing_defect_changes_the_gpu_tests_frames(cases, defect):
    caught = set()
    for name, (frames, frame_no, marks, timeline, strip, right) in cases.items():
        if not torch.equal(au.annotate_alt(frames, frame_no, marks, timeline, strip, defect=defect), right):
            caught.add(name)
    print(f"\n{defect}: caught by {sorted(caught)}")
    assert MUST[defect] <= caught, MUST[defect] - caught


def test_without_a_defect_nothing_differs(cases):
    for name, (frames, frame_no, marks, timeline, strip, right) in cases.items():
        assert torch.equal(au.annotate_alt(frames, frame_no, marks, timeline, strip), right), name
        assert torch.equal(au.annotate_ref(frames, frame_no, [], None, 0), frames), name
