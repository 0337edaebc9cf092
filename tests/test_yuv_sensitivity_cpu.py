"""Would tests/test_yuv_gpu.py notice a ``gcv_yuv420_to_rgb`` or ``gcv_rgb_to_yuv420`` that is subtly wrong?  Answered without
a GPU, as tests/test_quality_sensitivity_cpu.py does for its kernel: the GPU test compares bit for bit against
``yuvutil.to_rgb_ref`` / ``to_yuv_ref`` on the cases of tests/yuvutil.py under every layout, matrix and range, so a defect is
caught exactly when a restatement WITH that defect differs from the right one on one of those.  ``DEFECTS_IN`` and
``DEFECTS_OUT`` name, per defect, the comparisons that must each catch it.  A defect that stops differing is fixed by the
inputs, never by dropping it."""
import itertools

import numpy as np
import pytest

from tests import yuvutil as yu

INBOUND = ("uv_swap", "nv21", "nv12_as_i420", "chroma_row_y", "chroma_col_x", "u_stride_w", "v_at_u", "frame_stride_hw",
           "no_round", "no_clip", "no_low_clip", "oy_kept", "oy_dropped", "bt601_under_bt709", "lower_row_upper_y", "drop_tail",
           "g_v_sign")
OUTBOUND = ("topleft", "no_round_c", "no_oy", "rb_swap", "v_at_u", "nv21", "odd_rows_y", "no_clip_c", "drop_tail")
COMBOS = list(itertools.product(yu.LAYOUTS, yu.MATRICES, yu.RANGES))


def test_every_defect_is_audited():
    assert set(yu.DEFECTS_IN) == set(INBOUND) and len(INBOUND) == 17
    assert set(yu.DEFECTS_OUT) == set(OUTBOUND) and len(OUTBOUND) == 9
    for table, cases in ((yu.DEFECTS_IN, yu.SMALL_IN), (yu.DEFECTS_OUT, yu.SMALL_OUT)):
        for name, (what, where) in table.items():
            assert what and where and all(w[0] in cases and w[1:] in COMBOS for w in where), name


@pytest.mark.parametrize("defect", INBOUND)
def test_an_inbound_defect_changes_what_the_gpu_test_compares(defect):
    what, where = yu.DEFECTS_IN[defect]
    missed = [w for w in where if np.array_equal(yu.to_rgb_with(yu.case_in(w[0], w[1]), *w[1:], defect=defect),
                                                 yu.to_rgb_ref(yu.case_in(w[0], w[1]), *w[1:]))]
    print(f"\n{defect} ({what}): {len(where)} comparisons must catch it, {len(missed)} do not")
    assert not missed, missed


@pytest.mark.parametrize("defect", OUTBOUND)
def test_an_outbound_defect_changes_what_the_gpu_test_compares(defect):
    what, where = yu.DEFECTS_OUT[defect]
    missed = [w for w in where if np.array_equal(yu.to_yuv_with(yu.case_out(w[0]), *w[1:], defect=defect),
                                                 yu.to_yuv_ref(yu.case_out(w[0]), *w[1:]))]
    print(f"\n{defect} ({what}): {len(where)} comparisons must catch it, {len(missed)} do not")
    assert not missed, missed


def test_without_a_defect_nothing_differs():
    for name, combo in itertools.product(yu.SMALL_IN, COMBOS):
        yuv = yu.case_in(name, combo[0])
        assert np.array_equal(yu.to_rgb_with(yuv, *combo), yu.to_rgb_ref(yuv, *combo))
    for name, combo in itertools.product(yu.SMALL_OUT, COMBOS):
        assert np.array_equal(yu.to_yuv_with(yu.case_out(name), *combo), yu.to_yuv_ref(yu.case_out(name), *combo))


def test_the_inputs_hold_what_the_defects_need():
    """Both clips of every channel are driven by the random bytes and the table; the step case sits on both sides of the
    chroma rounding step; the flat case reaches the chroma clip under full range."""
    for matrix, full in itertools.product(yu.MATRICES, yu.RANGES):
        y, u, v = (p.astype(np.int64) for p in yu.planes(yu.case_in("table", "i420"), "i420"))
        up = lambda c: np.repeat(np.repeat(c, 2, 1), 2, 2)
        oy, cy, crv, cgu, cgv, cbu = yu.COEF_IN[(matrix, full)]
        lum = cy * (y - oy) + 8192
        for raw in ((lum + crv * (up(v) - 128)) >> 14, (lum + cgu * (up(u) - 128) + cgv * (up(v) - 128)) >> 14,
                    (lum + cbu * (up(u) - 128)) >> 14):
            assert raw.min() < 0 and raw.max() > 255
        s = yu.case_out("steps").astype(np.int64).reshape(1, 16, 2, 16, 2, 3).sum(axis=(2, 4))
        ur, ug, ub = yu.COEF_OUT[(matrix, full)][2]
        res = (ur * s[..., 0] + ug * s[..., 1] + ub * s[..., 2] + 32768) % 65536
        assert (res < 600).sum() >= 32 and (res >= 65536 - 600).sum() >= 32
    assert min(abs(c) for key in yu.COEF_OUT for row in yu.COEF_OUT[key][2:] for c in row) > 600      # one grey level crosses
    blue = np.asarray([[0, 0, 255]])
    assert int(yu._yuv_arith(blue, 4 * blue, yu.COEF_OUT[("bt709", True)], clip=False)[1][0]) == 0      # 256 wrapped
    assert int(yu.flat_yuv(blue, "bt709", True)[1][0]) == 255
