"""Would tests/test_cuts_gpu.py notice a ``gcv_frame_hist`` or ``gcv_hist_diff`` that is subtly wrong?  Answered without a
GPU, as tests/test_extend_sensitivity_cpu.py does for its kernel: the GPU test compares bit for bit against
``cutsutil.frame_hist_ref`` and ``hist_diff_ref`` on the videos of tests/cutsutil.py, so a defect is caught exactly when a
restatement WITH that defect differs from the right one somewhere on those inputs.  A defect that stops differing is fixed
by the inputs, never by dropping it.  The lag defects of ``hist_diff_lag`` ("lag ignored" cannot show at lag 1) are audited
in tests/test_transitions_sensitivity_cpu.py, beside the GPU test that launches lags."""
import numpy as np
import pytest

from tests import cutsutil as cu


def _cases():
    """name -> (frames, regions): every frame_hist launch of the GPU test (each followed by hist_diff)"""
    cases = {}
    shots, noise = cu.three_shot_video(), cu.noise_video()
    for r in (1, 2, 4, 8):
        cases[f"three shots R{r}"] = (shots, r)
        cases[f"noise R{r}"], cases[f"noise[1:] R{r}"], cases[f"noise[3:] R{r}"] = (noise, r), (noise[1:], r), (noise[3:], r)
    cases["many R4"], cases["tiny R8"] = (cu.many_video(), 4), (cu.tiny_video(), 8)
    cases["flat R1"], cases["flat R4"] = (cu.flat_pair(), 1), (cu.flat_pair(), 4)
    cases["striped R1"], cases["striped R2"] = (cu.striped_pair(), 1), (cu.striped_pair(), 2)
    cases["ends R1"], cases["ends R2"] = (cu.ends_pair(), 1), (cu.ends_pair(), 2)
    return cases


@pytest.fixture(scope="module")
def cases():
    out = {}
    for name, (frames, regions) in _cases().items():
        hist = cu.frame_hist_ref(frames, regions)
        out[name] = (frames, regions, hist, cu.hist_diff_ref(hist))
    return out


SPLIT = {"three shots R1", "three shots R2", "three shots R4", "noise R1", "noise[1:] R2", "flat R1", "flat R4", "striped R2"}
MUST = {                                                     # the cases that have to catch each defect
    "luma without rounding": {"three shots R1", "three shots R8", "noise R4", "many R4", "tiny R8"},
    "region edges rounded": {"three shots R4", "three shots R8", "noise R2", "noise R8", "many R4"},
    "regions transposed": {"three shots R2", "three shots R8", "noise R4", "many R4", "tiny R8"},
    "a row's last partial group dropped": {"three shots R1", "three shots R8", "noise R1", "noise[1:] R8", "many R4", "flat R4"},
    "a row's last partial group counted as four pixels": {"three shots R2", "three shots R8", "noise R4", "many R4", "flat R4"},
    "the byte-wise groups dropped": {"three shots R1", "noise R8", "noise[1:] R4", "noise[3:] R1", "many R4", "flat R1"},
    "the slice-boundary row counted twice": SPLIT,
    "the slice-boundary row dropped": SPLIT,
    "counts truncated to 16 bits": {"flat R1"},
    "bin 63 left out of the distance": {"ends R1", "ends R2"},
    "a - b without the absolute value": {"three shots R4", "noise R1", "many R4", "tiny R8", "flat R1", "striped R2", "ends R1"},
    "the second frame lag regions on": {"three shots R2", "three shots R8", "noise R4", "many R4", "flat R4", "ends R2"},
}
LAG_ONLY = {"lag ignored"}                                   # tests/test_transitions_sensitivity_cpu.py


def test_every_defect_is_audited():
    assert set(MUST) | LAG_ONLY == set(cu.HIST_DEFECTS) | set(cu.DIFF_DEFECTS) and len(MUST) == 12


@pytest.mark.parametrize("defect", sorted(MUST))
def test_a_defect_changes_what_the_gpu_test_compares(cases, defect):
    caught = set()
    for name, (frames, regions, hist, dist) in cases.items():
        if defect in cu.HIST_DEFECTS:
            differs = not np.array_equal(cu.frame_hist_alt(frames, regions, defect=defect), hist)
        else:
            differs = not np.array_equal(cu.hist_diff_alt(hist, 1, defect=defect), dist)
        if differs:
            caught.add(name)
    print(f"\n{defect}: caught by {sorted(caught)}")
    assert MUST[defect] <= caught, MUST[defect] - caught


def test_without_a_defect_nothing_differs(cases):
    for name, (frames, regions, hist, dist) in cases.items():
        assert np.array_equal(cu.frame_hist_alt(frames, regions), hist), name
        assert np.array_equal(cu.hist_diff_alt(hist), dist), name


def test_the_inputs_hold_what_the_gpu_test_says(cases):
    S = {name: cu.hist_slices(c[0].shape[0], c[0].shape[1], c[1]) for name, c in cases.items()}
    assert [S[f"three shots R{r}"] for r in (1, 2, 4, 8)] == [11, 5, 2, 1]          # split at R = 1, 2, 4; its own at R = 8
    assert {name for name, s in S.items() if s > 1} >= SPLIT
    frames = cases["three shots R1"][0]
    assert frames.shape == (15, 90, 130, 3) and 390 % 4 and all(90 % r and 130 % r for r in (4, 8))
    noise = cases["noise R8"][0]
    assert noise.shape == (4, 37, 53, 3) and (37 * 53 * 3) % 2 == 1                 # frames[1:] starts at an odd byte
    assert {int(n) for n in cu.region_pixels(37, 53, 8)} == {24, 28, 30, 35}        # 4-5 x 6-7 pixels: less than a wave
    many, r = cases["many R4"][:2]
    assert many.shape[0] * r * r == 1120 >= cu.FH_TARGET_WGS and S["many R4"] == 1
    assert cases["tiny R8"][0].shape == (2, 8, 8, 3) and int(cases["tiny R8"][2].max()) == 1
    assert int(cases["flat R1"][2].max()) == 67600 > 2 ** 16 and cases["flat R1"][3].tolist() == [[135200]]
    hist = cases["striped R1"][2]
    assert hist[0, 0, 10] == 64 * 96 and hist[1, 0, 10] == hist[1, 0, 62] == 32 * 96
    hist = cases["ends R1"][2]
    assert hist[0, 0, 63] == 16 * 24 and hist[1, 0, 63] == 16 * 8 and hist[1, 0, 0] == 16 * 16
