"""gcv_k_dwconv7_ln2 — two image groups of the depthwise 7x7 + LayerNorm in one launch (csrc/dwconv_impl.h,
launch_dwconv7_ln2) — against two gcv_k_dwconv7_ln calls of the same library on the same inputs.  Each group of the merged
launch runs the device code of its single launch under the same plan, so the comparison is torch.equal, not a tolerance.

The map sizes are those of ConvNeXt-T's 224- + 112-pixel pass (the VAE's), stage by stage.  Stages 1 - 3 have a merged
kernel; stage 0 (C = 96) and every pair outside the table take two launches inside gcv_k_dwconv7_ln2 and must match all the
same.  Both groups live in one buffer, group 1 behind group 0 as in the network's token stream, with a sentinel image behind
each group's output: a workgroup that took the other group's geometry or index would write there or leave zeros.

Those image counts plan the short bands of small launches.  The bands of the VAE's real batches (14- and 7-row bands at B = 128)
are reached with two images per group through gcv_k_dwconv7_ln2_planned / gcv_k_dwconv7_ln_planned, which take the plan of a
larger image count: every pair of band geometries that pass reaches at any batch (tests/dwcases.py MERGED)."""
import ctypes

import pytest
import torch

from genconvit_amd import _lib
from tests import dwcases, kutil
from tests.kutil import DTYPES, dev, ptr, rnd

pytestmark = pytest.mark.gpu
torch.set_grad_enabled(False)

DW_KINDS = ("tile", "tiny", "tiny_pair", "roll", "mfma", "pair")      # gcv_dw_plan's kind codes (include/genconvit_hip.h)
# (C, side of group 0, side of group 1, kinds gcv_dw_plan names for them at these image counts)
STAGES = [(96, 56, 28, ("roll", "roll")), (192, 28, 14, ("roll", "roll")), (384, 14, 7, ("roll", "roll")),
          (768, 7, 3, ("roll", "tiny"))]
COUNTS = [(2, 2), (3, 1), (1, 3)]                  # both grid halves, their boundary, unequal counts either way
SENTINEL = 7.0


def _plan_kind(dtype, n, H, W, C):
    out = (ctypes.c_int * 5)()
    _lib.check(_lib.load().gcv_dw_plan(_lib.dtype_code(dtype), n, H, W, C, 1, out), "gcv_dw_plan")
    return DW_KINDS[out[0]]


def _params(C, seed):
    wdw = rnd((49, C), seed, 1.0 / 7.0).to(dev())
    return wdw, rnd((C,), seed + 1, 0.2).to(dev()), (1.0 + rnd((C,), seed + 2, 0.3)).to(dev()), rnd((C,), seed + 3, 0.3).to(dev())


def _merged_vs_single(dtype, C, geo0, geo1, seed=0, plan=None):
    """geo = (n, H, W).  Returns nothing; asserts the merged launch's outputs equal the two single launches' bit for bit.
    plan = (plan_nimg0, plan_nimg1): both sides through the *_planned entries, each group under the plan of that many images."""
    (n0, H0, W0), (n1, H1, W1) = geo0, geo1
    e0, e1 = n0 * H0 * W0 * C, n1 * H1 * W1 * C
    assert e0 % 8 == 0 and e1 % 8 == 0              # both groups 16-byte aligned inside the one buffer
    x = rnd((e0 + e1,), 100 + seed, 2.0).to(dev(), dtype)
    wdw, b, lw, lb = _params(C, 200 + seed)
    pad0, pad1 = -(H0 * W0 * C) % 8 + H0 * W0 * C, -(H1 * W1 * C) % 8 + H1 * W1 * C     # one sentinel image behind each group
    outs = []
    for merged in (False, True):
        y = torch.full((e0 + pad0 + e1 + pad1,), SENTINEL, dtype=dtype, device=dev())
        x0, x1, y0, y1 = x[:e0], x[e0:], y[:e0], y[e0 + pad0:]
        assert all(t.data_ptr() % 16 == 0 for t in (x0, x1, y0, y1))
        dt = _lib.dtype_code(dtype)
        if merged and plan:
            kutil.call("gcv_k_dwconv7_ln2_planned", dt, ptr(x0), ptr(y0), n0, H0, W0, ptr(x1), ptr(y1), n1, H1, W1, ptr(wdw),
                       ptr(b), ptr(lw), ptr(lb), C, 1e-6, plan[0], plan[1])
        elif plan:
            kutil.call("gcv_k_dwconv7_ln_planned", dt, ptr(x0), ptr(wdw), ptr(b), ptr(lw), ptr(lb), ptr(y0), n0, H0, W0, C, 1e-6,
                       plan[0])
            kutil.call("gcv_k_dwconv7_ln_planned", dt, ptr(x1), ptr(wdw), ptr(b), ptr(lw), ptr(lb), ptr(y1), n1, H1, W1, C, 1e-6,
                       plan[1])
        elif merged:
            kutil.call("gcv_k_dwconv7_ln2", dt, ptr(x0), ptr(y0), n0, H0, W0, ptr(x1), ptr(y1), n1, H1, W1, ptr(wdw), ptr(b),
                       ptr(lw), ptr(lb), C, 1e-6)
        else:
            kutil.call("gcv_k_dwconv7_ln", dt, ptr(x0), ptr(wdw), ptr(b), ptr(lw), ptr(lb), ptr(y0), n0, H0, W0, C, 1e-6)
            kutil.call("gcv_k_dwconv7_ln", dt, ptr(x1), ptr(wdw), ptr(b), ptr(lw), ptr(lb), ptr(y1), n1, H1, W1, C, 1e-6)
        assert (y[e0:e0 + pad0].float() == SENTINEL).all() and (y[e0 + pad0 + e1:].float() == SENTINEL).all(), \
            f"merged={merged}: written outside the images"
        outs.append(y)
    single, two = outs
    assert torch.isfinite(single.float()).all() and (single[:e0].float() != SENTINEL).any() and \
        (single[e0 + pad0:e0 + pad0 + e1].float() != SENTINEL).any()
    assert torch.equal(two[:e0], single[:e0]), f"group 0: {int((two[:e0] != single[:e0]).sum())} of {e0} values differ"
    assert torch.equal(two, single), "group 1 differs"


@pytest.mark.parametrize("dt", ["f16", "bf16"])
@pytest.mark.parametrize("n0,n1", COUNTS)
@pytest.mark.parametrize("C,S0,S1,kinds", STAGES)
def test_two_group_launch_matches_two_launches(dt, n0, n1, C, S0, S1, kinds):
    """The four stages of the 224- + 112-pixel pass at image counts (2, 2), (3, 1), (1, 3)."""
    dtype = DTYPES[dt]
    assert (_plan_kind(dtype, n0, S0, S0, C), _plan_kind(dtype, n1, S1, S1, C)) == kinds
    _merged_vs_single(dtype, C, (n0, S0, S0), (n1, S1, S1), seed=C + n0)


@pytest.mark.parametrize("dt", ["f32", "f16", "bf16"])
@pytest.mark.parametrize("C,H0,H1,plan0,plan1", dwcases.MERGED)
def test_two_group_launch_at_every_pair_of_band_geometries(dt, C, H0, H1, plan0, plan1):
    """Two images per group under the plans of the VAE's merged 224- + 112-pixel pass at the batch plan0 = plan1: every pair of
    (kernel, H, rows per band) that pass reaches at B = 1 ... 512 (tests/dwcases.py MERGED, held against the census of the
    networks' launches by tests/test_host_cpu.py), against two gcv_k_dwconv7_ln_planned launches under the same plans.
    The single launches under those plans are compared with the float64 reference in tests/test_kernels_gpu.py."""
    dtype = DTYPES[dt]
    out = (ctypes.c_int * 1)()
    _lib.check(_lib.load().gcv_dw_plan2(_lib.dtype_code(dtype), plan0, H0, H0, plan1, H1, H1, C, out), "gcv_dw_plan2")
    assert out[0] == 1, "these plans do not merge"
    _merged_vs_single(dtype, C, (2, H0, H0), (2, H1, H1), seed=C + plan0, plan=(plan0, plan1))


@pytest.mark.parametrize("dt", ["f16", "bf16"])
def test_two_group_launch_with_the_mfma_kernel_in_front(dt):
    """64 + 64 images at C = 96: 64 x 56 image rows is kDwMfmaMinImageRows, so group 0 is the matrix-pipe kernel."""
    dtype = DTYPES[dt]
    assert (_plan_kind(dtype, 64, 56, 56, 96), _plan_kind(dtype, 64, 28, 28, 96)) == ("mfma", "roll")
    _merged_vs_single(dtype, 96, (64, 56, 56), (64, 28, 28), seed=9)


@pytest.mark.parametrize("dt", ["f16", "bf16"])
@pytest.mark.parametrize("C,geo0,geo1,kinds", [
    (768, (2, 7, 7), (2, 5, 5), ("roll", "tile")),             # W = 5: the generic tile kernel behind a band kernel
    (192, (2, 14, 14), (2, 28, 28), ("roll", "roll")),         # a covered pair in the other order
    (768, (2, 7, 7), (3, 4, 4), ("roll", "tiny")),             # Tiny at an S without a merged kernel
])
def test_pairs_outside_the_table_fall_back_to_two_launches(dt, C, geo0, geo1, kinds):
    dtype = DTYPES[dt]
    assert (_plan_kind(dtype, *geo0, C), _plan_kind(dtype, *geo1, C)) == kinds
    _merged_vs_single(dtype, C, geo0, geo1, seed=C + geo1[1])
