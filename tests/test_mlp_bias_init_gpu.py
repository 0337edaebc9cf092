"""b2 of the narrow-stage fused ConvNeXt MLP kernels, made visible: a bias that is dropped, added twice, or handled once per
workgroup instead of once per token tile / pass must show.  So b2 is large here (|b2| in [2, 4], against 0.1 in the other
fused-MLP cases) and |gamma| is at least 0.05: a wrong bias moves an output by at least 0.05 * 2 = 0.1, far outside the
tolerances, which are the ones the existing fused-MLP kernel cases use (tests/kutil.py: tol(dtype, 2) for the residual
stream, tol(dtype, 4) behind the LayerNorm-patchify epilogue).  Reference: plain fp32 torch on inputs rounded to the
storage dtype, the hidden activation rounded to it as the kernels do, as in tests/test_kernels_gpu.py.  The kernels add b2
in the epilogue today; the cases are the ones a kernel that starts GEMM2's accumulator at b2 has to pass as well.

Which kernel a shape reaches (cnx_mlp.h, fused_mlp.h): C = 96 runs fused_mlp_res_kernel from 65 536 tokens on and
fused_mlp_kernel<T, 96, 4> below; the LN-patchify epilogue exists at C = 96 only in the former (the entry refuses it below
65 536 tokens).  C = 192 always runs xs_mlp_kernel, on min(passes, 256) workgroups of one 256-token pass each, so a
workgroup sees a second pass from 65 537 tokens on.  The small shapes therefore check the bias on the first tile / pass,
ragged, and the shapes just above 65 536 tokens are the ones in which a wave runs a second tile (C = 96: 2 065 tiles on
2 048 waves) or a workgroup a second pass (C = 192: 258 passes on 256 workgroups; xs_mlp_kernel's accumulators start again
from the inline zero of the peeled first steps).  The small LN-patchify geometries (two images of 4 x 4 and of 6 x 6 tokens)
run alone at C = 192 and as the trailing segment behind 21 images of 56 x 56 at C = 96."""
import ctypes
import math

import pytest
import torch
import torch.nn.functional as F

from genconvit_amd import _lib
from tests import kutil
from tests.kutil import DTYPES, dev, ptr, rnd, tol

pytestmark = pytest.mark.gpu
torch.set_grad_enabled(False)


def q(t, dtype):
    return t.to(dtype).float()


def _signed(shape, seed, lo, hi):
    """uniform in +-[lo, hi]"""
    u = rnd(shape, seed)                                   # U(-1, 1): the sign, and |u| for the magnitude
    return torch.sign(u + (u == 0).float()) * (lo + (hi - lo) * u.abs())


def _inputs(C, M, dtype):
    x = q(rnd((M, C), 1, 1.5), dtype)
    w1 = q(rnd((4 * C, C), 2, 1 / math.sqrt(C)), dtype)
    w2 = q(rnd((C, 4 * C), 3, 1 / math.sqrt(4 * C)), dtype)
    b1 = rnd((4 * C,), 4, 0.1)
    b2 = _signed((C,), 5, 2.0, 4.0)
    gamma = _signed((C,), 6, 0.05, 0.5)                    # U(-0.5, 0.5) without |gamma| < 0.05
    res = q(rnd((M, C), 7), dtype)
    h = q(F.gelu(x @ w1.t() + b1), dtype)                  # the kernels round the hidden activation to T for GEMM2
    y = res + gamma * (h @ w2.t() + b2)
    assert b2.abs().min() >= 2.0 and gamma.abs().min() >= 0.05
    return x, w1, w2, b1, b2, gamma, res, y


def _report(name, got, want, bound):
    err = (got.float().cpu() - want).abs().max().item()
    print(f"{name}: max |diff| = {err:.3e} (bound {bound:.3e})")
    assert err <= bound, f"{name}: max |diff| {err:.3e} > {bound:.3e}"


@pytest.mark.parametrize("dt", ["bf16", "f16"])
@pytest.mark.parametrize("C,M", [
    (96, 33), (96, 8 * 32 * 2 + 1),        # one token past a 32-token tile; 513 tokens (fused_mlp_kernel<T, 96, 4>)
    (96, 65536 + 8 * 32 * 2 + 1),          # fused_mlp_res_kernel: 2 065 tiles on 2 048 waves, the last one ragged
    (192, 257), (192, 513),                # xs_mlp_kernel: 2 / 3 workgroups, ragged last pass
    (192, 65536 + 257),                    # 258 passes on 256 workgroups: second pass, the last one ragged
])
def test_bias_initialised_accumulator(dt, C, M):
    dtype = DTYPES[dt]
    x, w1, w2, b1, b2, gamma, res, want = _inputs(C, M, dtype)
    D = lambda t, d=None: t.to(dev()) if d is None else t.to(dev(), d)
    xd, w1d, b1d, w2d, b2d, gd = D(x, dtype), D(w1, dtype), D(b1), D(w2), D(b2), D(gamma)
    out = torch.full((M + 8, C), 7.0, dtype=dtype, device=dev())
    out[:M] = res.to(dev(), dtype)
    kutil.call("gcv_k_fused_mlp", _lib.dtype_code(dtype), C, ptr(xd), ptr(w1d), ptr(b1d), ptr(w2d), ptr(b2d), ptr(gd),
               ptr(out), ptr(out), M)
    assert (out[M:].float() == 7.0).all(), "rows past M were written"
    _report(f"fused mlp, b2 in +-[2, 4], C={C} M={M} {dt}", out[:M], want, tol(dtype, 2.0))


# segments: (images, H, W) per segment, in token order
_LNP = [
    (96, [(21, 56, 56), (2, 4, 4)]),       # 65 856 + 32 tokens: the two 4 x 4 images are one tile, some wave's second
    (96, [(21, 56, 56), (2, 6, 6)]),       # 65 856 + 72: two full tiles and a ragged one of 8 tokens
    (192, [(2, 4, 4)]),                    # 32 tokens
    (192, [(2, 6, 6)]),                    # 72 tokens
    (192, [(84, 28, 28), (2, 6, 6)]),      # 65 856 + 72: 258 passes on 256 workgroups, the second pass holds the 6 x 6 images
]


@pytest.mark.parametrize("dt", ["bf16", "f16"])
@pytest.mark.parametrize("C,segs", _LNP)
def test_bias_initialised_accumulator_layernorm_patchify(dt, C, segs):
    dtype = DTYPES[dt]
    M = sum(n * h * w for n, h, w in segs)
    x, w1, w2, b1, b2, gamma, res, y = _inputs(C, M, dtype)
    lw, lb = rnd((C,), 8, 0.5) + 1.0, rnd((C,), 9, 0.1)
    yn = F.layer_norm(y, (C,), lw, lb, 1e-6)
    want, tok0, hw, wd, out0, t = [], [], [], [], [], 0
    for n, H, W in segs:
        tok0.append(t); hw.append(H * W); wd.append(W); out0.append(t // 4)
        v = yn[t:t + n * H * W].reshape(n, H // 2, 2, W // 2, 2, C).permute(0, 1, 3, 2, 4, 5)
        want.append(v.reshape(n * (H // 2) * (W // 2), 4 * C))
        t += n * H * W
    want = torch.cat(want)
    D = lambda t, d=None: t.to(dev()) if d is None else t.to(dev(), d)
    xd, w1d, b1d, w2d, b2d, gd, lwd, lbd = D(x, dtype), D(w1, dtype), D(b1), D(w2), D(b2), D(gamma), D(lw), D(lb)
    resd = D(res, dtype)
    out = torch.full((M // 4 + 3, 4 * C), 7.0, dtype=dtype, device=dev())
    arr = lambda v: (ctypes.c_int * 4)(*(v + [0] * (4 - len(v))))
    a_tok0, a_hw, a_wd, a_out0 = arr(tok0), arr(hw), arr(wd), arr(out0)
    kutil.call("gcv_k_fused_mlp_lnp", _lib.dtype_code(dtype), C, ptr(xd), ptr(w1d), ptr(b1d), ptr(w2d), ptr(b2d), ptr(gd),
               ptr(resd), ptr(lwd), ptr(lbd), 1e-6, len(segs), a_tok0, a_hw, a_wd, a_out0, ptr(out), M)
    assert torch.equal(resd.cpu(), res.to(dtype)), "the residual stream must not be written"
    assert (out[M // 4:].float() == 7.0).all(), "rows behind the last patch row were written"
    _report(f"fused mlp + LN-patchify, b2 in +-[2, 4], C={C} {segs} {dt}", out[:M // 4], want, tol(dtype, 4.0))
