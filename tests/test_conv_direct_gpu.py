"""The direct 3x3 convolution kernel for 16-bit storage (csrc/conv_direct.h), reached through gcv_k_gemm exactly as the
networks reach it: gemm_select (csrc/gemm_impl.h) sends the A_IM2COL3_POOL / EPI_POOL4 launches with Cin = 16 / 32, N = 32 / 64
and the A_IM2COL3_S2 / EPI_BIAS_ACT launches with Cin = 16, N = 32 / 64 there, and everything else
to gemm_kernel (tests/gemmcases.py has the cases and the kernel each reaches; tests/test_host_cpu.py asserts it): the stride-2 cases at Cin = 32 below pin that generic path, which measured faster for them.  Inputs, float64
reference and comparator are tests/kcases.py's conv3x3_pool / conv3x3_s2, unchanged.

A wave's work item is 32 consecutive rows m of the flattened launch x 32 output channels, and the launcher starts
min(1024, ceil(items / 8)) workgroups of four waves (DirectShape, csrc/gemm_impl.h), so a wave makes two trips of its loop wherever there
are eight items or more, the second block's loads issued beside the first block's MFMAs:
  pool (1, 2, 16, 32)    4 rows: one window, one partial block; five of the nine taps of every pixel fall outside the image
  pool (3, 6, 16, 32)    108 rows = 27 windows, 9 per image: blocks straddle image rows and images, the fourth block has 12
                         rows; one trip
  pool (3, 6, 32, 64)    the same rows, two channel blocks on neighbouring waves: two waves per channel block, two trips each
  pool (2, 16, 32, 64)   512 rows, 32 items, 4 workgroups: two trips
  s2   (1, 2, 32, 64)    one output pixel (gemm_kernel)
  s2   (5, 6, 16, 32)    45 output pixels: the second block has 13 rows
  s2   (5, 6, 32, 64)    the same at Cin = 32 (gemm_kernel)
  (2, 16, 16, 16)        N = 16, both modes: stays on gemm_kernel's 32-deep-K instances
The long loop is tests/test_kernels_gpu.py's pool case (3, 112, 16, 32): 37632 rows = 1176 items -> 147 workgroups, 588 waves,
two trips each.  (At the network's 128 frames the grid is capped: 50176 items on 4096 waves, 12 or 13 trips.)

Every case writes into the middle of a buffer filled with a sentinel: guard rows in front of and behind the result and eight
padding columns per row must come back untouched."""
import math

import pytest
import torch

from genconvit_amd import _lib
from tests import gemmcases, kcases
from tests.kutil import DTYPES, dev, gemm

pytestmark = pytest.mark.gpu
torch.set_grad_enabled(False)

SENTINEL = 7.0
GUARD = gemmcases.DIRECT_GUARD      # rows in front of and behind the result
PAD = gemmcases.DIRECT_PAD          # columns behind the result: ldc stays a multiple of 8 (the stride-2 epilogue stores 16-byte pieces)


def _run(case, mode, n, H, cin, cout, dtype):
    x, w, b = (case.inputs[k] for k in ("x", "w", "b"))
    x_nhwc = x.permute(0, 2, 3, 1).contiguous().to(dev(), dtype)
    wt = w.permute(0, 2, 3, 1).reshape(cout, 9 * cin).contiguous().to(dev(), dtype)
    bias = b.to(dev())
    Ho = H // 2
    rows, ldc = n * Ho * Ho, cout + PAD
    buf = torch.full((GUARD + rows + GUARD, ldc), SENTINEL, dtype=dtype, device=dev())
    out = buf[GUARD:GUARD + rows]
    # what gemm_select asks of a launch before it takes the direct kernel's 16-byte stores
    assert out.data_ptr() % 16 == 0 and ldc % 8 == 0
    if mode == "pool":
        gemm(dtype, _lib.A_IM2COL3_POOL, _lib.EPI_POOL4, x_nhwc, wt, out, n * H * H, cout, 9 * cin, ldc=ldc,
             bias=bias, act=1, H=H, W=H, cin_log2=int(math.log2(cin)))
    else:
        gemm(dtype, _lib.A_IM2COL3_S2, _lib.EPI_BIAS_ACT, x_nhwc, wt, out, rows, cout, 9 * cin, ldc=ldc,
             bias=bias, act=3, H=H, W=H, cin_log2=int(math.log2(cin)))
    got = buf.float().cpu()
    assert torch.all(got[:GUARD] == SENTINEL), "rows in front of the result were written"
    assert torch.all(got[GUARD + rows:] == SENTINEL), "rows behind the result were written"
    assert torch.all(got[:, cout:] == SENTINEL), "padding columns were written"
    case.assert_close(out[:, :cout].reshape(n, Ho, Ho, cout))


@pytest.mark.parametrize("dt", ["f16", "bf16"])
@pytest.mark.parametrize("n,H,cin,cout", gemmcases.cases(gemmcases.DIRECT_POOL))
def test_direct_conv3x3_relu_maxpool(dt, n, H, cin, cout):
    dtype = DTYPES[dt]
    _run(kcases.conv3x3_pool(n, H, cin, cout, dtype), "pool", n, H, cin, cout, dtype)


@pytest.mark.parametrize("dt", ["f16", "bf16"])
@pytest.mark.parametrize("n,H,cin,cout", gemmcases.cases(gemmcases.DIRECT_S2))
def test_direct_conv3x3_stride2_leaky(dt, n, H, cin, cout):
    dtype = DTYPES[dt]
    _run(kcases.conv3x3_s2(n, H, cin, cout, dtype), "s2", n, H, cin, cout, dtype)
