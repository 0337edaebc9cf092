"""Would tests/test_persons_gpu.py notice a kernel that is subtly wrong?  Answered without a GPU, as
tests/test_kernel_sensitivity_cpu.py does for the network kernels: the GPU tests compare bit for bit against the
restatements of tests/personutil.py on ``signature_case`` and ``link_cases``, so a defect is caught exactly when a
restatement WITH that defect differs from the right one somewhere on those inputs.  Each defect below is one a kernel of
this shape could plausibly have; a defect that stops differing is fixed by the inputs, never by dropping it."""
import numpy as np
import pytest

from tests import personutil as pu

NONE = pu.NONE


# ----------------------------------------------------------------------------- gcv_face_signature
def _edge_up(extent, grid):
    """a cell edge off by one: rounded up instead of down (the same where grid divides i * extent)"""
    return np.array([-((-i * int(extent)) // grid) for i in range(grid + 1)], dtype=np.int64)


def _normalise_truncating(c):
    c = np.asarray(c, dtype=np.int64)
    d = 256 * c - c.sum()
    A = int(np.abs(d).sum())
    return np.full_like(c, 128) if A == 0 else np.clip(128 + np.sign(d) * ((8192 * np.abs(d)) // A), 0, 255)


def _normalise_unclamped(c):
    c = np.asarray(c, dtype=np.int64)
    d = 256 * c - c.sum()
    A = int(np.abs(d).sum())
    return np.full_like(c, 128) if A == 0 else 128 + np.sign(d) * ((8192 * np.abs(d) + A // 2) // A)     # the byte wraps


SIGNATURE_DEFECTS = {
    "a cell edge off by one": dict(edges=_edge_up),
    "cell means truncated": dict(mean=lambda sums, cnt: sums // cnt),
    "normalisation truncated": dict(normalise=_normalise_truncating),
    "no clamp": dict(normalise=_normalise_unclamped),
    "Cb and Cr swapped": dict(chroma=lambda frame: pu.chroma(frame)[::-1]),
}


@pytest.fixture(scope="module")
def signatures():
    frames, boxes = pu.signature_case()
    return frames, boxes, pu.face_signature_ref(frames, boxes)


@pytest.mark.parametrize("defect", sorted(SIGNATURE_DEFECTS))
def test_a_signature_defect_changes_the_gpu_tests_rows(signatures, defect):
    frames, boxes, right = signatures
    wrong = pu.face_signature_ref(frames, boxes, **SIGNATURE_DEFECTS[defect])
    rows = (wrong != right).any(1)
    print(f"\n{defect}: {int(rows.sum())} of {len(boxes)} rows differ, {int((wrong != right).sum())} bytes")
    assert rows.any()
    if defect == "no clamp":                                 # only the rows that clamp can show it: the two on the stripes do
        assert rows[12] and rows[13]
    if defect == "a cell edge off by one":                   # the box of side 16 cannot (every edge is exact), 17 x 23 must
        assert not rows[0] and rows[1]


def test_the_signature_inputs_hold_what_the_gpu_test_says(signatures):
    frames, boxes, right = signatures
    sides = [(b[3] - b[1], b[2] - b[4]) for b in boxes]
    assert sides[0] == (16, 16) and sides[1] == (17, 23) and sides[2] == (16, 100) and sides[3] == (90, 16)
    assert (96, 128) in sides and min(b[1] for b in boxes) == 0 and min(b[4] for b in boxes) == 0
    assert max(b[3] for b in boxes) == 96 and max(b[2] for b in boxes) == 128
    assert (right[10, :256] == 128).all() and right[12, :256].max() == 255 and right[13, :256].min() == 0


# ----------------------------------------------------------------------------- gcv_sig_link
def _skips_the_last_partial_tile(sig, owner, T):
    n = (len(owner) // 64) * 64
    return pu.sig_link_ref(sig[:n], owner[:n], T)


def _skips_rows_from_64(sig, owner, T):
    return pu.sig_link_ref(sig[:64], owner[:64], T)


def _ignores_owner_minus_one(sig, owner, T):
    """a row marked -1 lands where the index -1 lands: in the last track"""
    return pu.sig_link_ref(sig, [o % T for o in owner], T)


def _writes_one_triangle(sig, owner, T):
    out = pu.sig_link_ref(sig, owner, T)
    out[np.tril_indices(T, -1)] = NONE
    return out


LINK_DEFECTS = {
    # (n = 1 cannot show anything: one row has no pair, it is there for the launch of a lone, nearly empty tile)
    "skips the last partial tile": (_skips_the_last_partial_tile, {"n=63", "n=65", "n=130", "unsorted", "equal rows"}),
    "skips rows from 64 on": (_skips_rows_from_64, {"n=65", "n=130", "unsorted", "equal rows"}),
    "ignores owner -1": (_ignores_owner_minus_one, {"owner -1"}),
    "writes one triangle only": (_writes_one_triangle, {"n=63", "n=64", "n=65", "n=130", "0 against 255"}),
}


@pytest.mark.parametrize("defect", sorted(LINK_DEFECTS))
def test_a_link_defect_changes_the_gpu_tests_matrices(defect):
    wrong, must = LINK_DEFECTS[defect]
    caught = set()
    for name, sig, owner, T in pu.link_cases():
        if not np.array_equal(wrong(sig, list(owner), T), pu.sig_link_ref(sig, owner, T)):
            caught.add(name)
    print(f"\n{defect}: caught by {sorted(caught)}")
    assert must <= caught, must - caught


def test_the_link_inputs_hold_what_the_gpu_test_says():
    cases = {name: (sig, owner, T) for name, sig, owner, T in pu.link_cases()}
    assert [len(cases[f"n={n}"][1]) for n in (1, 63, 64, 65, 130)] == [1, 63, 64, 65, 130]
    owner = cases["n=130"][1]
    starts = [owner.index(t) for t in range(5)]
    assert owner == sorted(owner) and all(s % 64 for s in starts[1:]) and len({owner.count(t) for t in range(5)}) == 5
    assert cases["unsorted"][1] != sorted(cases["unsorted"][1]) and -1 in cases["owner -1"][1]
    assert 2 not in cases["empty track"][1] and cases["empty track"][2] == 4 and cases["T=1"][2] == 1
    assert pu.sig_link_ref(*cases["equal rows"])[0, 1] == 0 and pu.sig_link_ref(*cases["0 against 255"])[0, 1] == 97920
