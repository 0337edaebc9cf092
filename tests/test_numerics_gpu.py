"""Numerics off the benign input distribution (every other kernel test draws U(-1, 1) * scale): the GELU of every site that
evaluates one, swept over every finite value of the storage dtype through identity weights, and the LayerNorm of every
kernel that computes one, on rows with a large common offset, a tiny or large scale, and no variance at all, and the softmax
of the Swin window attention on uniform rows, on rows whose logits span 270, and where a masked key still wins.  References are
float64; the bounds (tests/numutil.py) are rounding terms plus a measured allowance, and tests/test_numerics_cpu.py shows
without a GPU that each of them rejects a defective restatement of the device formula.  Every case prints what it measured."""
import ctypes
import math

import pytest
import torch
import torch.nn.functional as F

from genconvit_amd import _lib
from tests import gemmcases, kutil, numutil as nu
from tests.kutil import DTYPES, dev, gemm, ptr, rnd

pytestmark = pytest.mark.gpu
torch.set_grad_enabled(False)

ALL = ["f32", "bf16", "f16"]
H16 = ["bf16", "f16"]
SENT = 7.0


def q(t, dtype):
    return t.to(dtype).float()


# ============================================================================= A. GELU sweeps
def _values(dt, offgrid):
    """shuffled 1-D value set of a storage dtype, in that dtype: on-grid every finite value (fp32 storage: both 16-bit grids,
    |x| <= 1e30), off-grid those of |x| <= 8 (a fp32 bias per column is added by the kernel)"""
    if dt == "f32":
        v = torch.cat([nu.finite_grid(torch.float16).float(), nu.finite_grid(torch.bfloat16).float()])
        v = v[v.abs() <= 1e30]
    else:
        v = nu.finite_grid(DTYPES[dt])
    if offgrid:
        v = v[v.float().abs() <= 8]
    return nu.shuffled(v)


def _delta(pre, nvalues, dtype, offgrid):
    """numutil.gelu_delta of a tiled (M, N) value set, taken over the rows after which its (value, bias column) pairs repeat:
    the same maximum as over all M rows, at a fraction of the fp16 emulation's cost for the 65 581-row case"""
    M, N = pre.shape
    return nu.gelu_delta(pre[:min(M, math.lcm(nvalues, N) // N)], dtype, offgrid)


def _judge_gelu(dt, offgrid, got, pre, what, delta):
    """got: the site's stored results (CPU), pre: the exact fp32 pre-activations, same shape; delta: _delta of pre (unused
    for fp32 storage)"""
    dtype = DTYPES[dt]
    got = got.double()
    assert torch.isfinite(got).all(), f"{what}: non-finite GELU of a finite input"
    if dt == "f32":
        want = nu.gelu_ref(pre)
        ratio = ((got - want).abs() / nu.gelu_f32_bound(pre, want).clamp(min=1e-300)).max().item()
        print(f"NUMERICS gelu {what} f32 {'off' if offgrid else 'on'}-grid: worst error / bound = {ratio:.3f}")
        assert ratio <= 1.0, f"{what}: fp32 GELU error is {ratio:.3f} of 6e-7 |x| + 2^-22 |want|"
        return
    ok, ex = nu.gelu_h16_holds(got, pre, dtype, offgrid, delta)
    print(f"NUMERICS gelu {what} {dt} {'off' if offgrid else 'on'}-grid: delta {delta:.4e} excess {ex:.4e}")
    assert ok, f"{what}: error beyond rounding {ex:.3e} > delta {delta:.3e}"


# (name, storage dtypes, M, N = K, ldc) from tests/gemmcases.py: one site per tile of the plain bias + activation launch and the
# LDS-DMA kernel, each asserted below through gcv_gemm_plan
_GEMM_SITES = gemmcases.cases(gemmcases.GELU_SITES)
_GEMM_KERNEL = {c[0]: k for c, k in gemmcases.GELU_SITES}


@pytest.mark.parametrize("offgrid", [False, True], ids=["ongrid", "offgrid"])
@pytest.mark.parametrize("site,dt", [(s, dt) for s in _GEMM_SITES for dt in s[1]], ids=lambda v: v if isinstance(v, str) else v[0])
def test_gelu_gemm_epilogue_over_every_value(site, dt, offgrid):
    """gcv_k_gemm, EPI_BIAS_ACT with GELU and Wt = I: the accumulator is A exactly, the pre-activation fp32(A + bias)."""
    name, _, M, N, ldc = site
    dtype = DTYPES[dt]
    launch = gemmcases.linear(M, N, N, _lib.ACT_GELU, ldc=ldc)
    assert gemmcases.plan(dt, launch)[:6] == gemmcases.resolve(_GEMM_KERNEL[name], dt)
    vals = _values(dt, offgrid)
    A = nu.tile_to(vals, M * N).reshape(M, N)
    bias = nu.offgrid_bias(N) if offgrid else torch.zeros(N)
    pre = A.float() + bias
    Ad, Wd, bd = A.to(dev()), torch.eye(N, dtype=dtype, device=dev()), bias.to(dev())
    C = torch.full((M + 8, ldc), SENT, dtype=dtype, device=dev())
    gemm(dtype, _lib.A_PLAIN, _lib.EPI_BIAS_ACT, Ad, Wd, C, M, N, N, lda=N, ldc=ldc, bias=bd, act=2)
    out = C.cpu()
    assert (out[M:].float() == SENT).all() and (out[:M, N:].float() == SENT).all(), "written outside the M x N result"
    _judge_gelu(dt, offgrid, out[:M, :N], pre, f"gemm {name}", None if dt == "f32" else _delta(pre, vals.numel(), dtype, offgrid))


# (name, C, M): fused_mlp_kernel<T, 96, 4> below 65 536 tokens, fused_mlp_res_kernel from there on (fused_mlp_res_applies),
# xs_mlp_kernel at C = 192, xs_pw1_kernel + pw2f_kernel at C = 384
_MLP_SITES = [("fused96", 96, 667), ("res96", 96, 65536 + 45), ("xs192", 192, 333), ("pair384", 384, 167)]


@pytest.mark.parametrize("offgrid", [False, True], ids=["ongrid", "offgrid"])
@pytest.mark.parametrize("dt", H16)
@pytest.mark.parametrize("site", _MLP_SITES, ids=lambda s: s[0])
def test_gelu_fused_mlp_hidden_over_every_value(site, dt, offgrid):
    """gcv_k_fused_mlp with fc1 a stack of four identities and fc2 the selector of hidden chunk k: out[m, c] is the stored
    hidden activation T(GELU(x[m, c] + b1[k C + c])) of hidden unit k C + c.  Four launches, k = 0 .. 3: every hidden chunk,
    hence the steady state and the drain / tail code of each kernel, is observed."""
    name, C, M = site
    dtype = DTYPES[dt]
    vals = _values(dt, offgrid)
    x = nu.tile_to(vals, M * C).reshape(M, C)
    b1 = nu.offgrid_bias(4 * C) if offgrid else torch.zeros(4 * C)
    w1 = torch.eye(C).repeat(4, 1)                                   # w1[j, j mod C] = 1
    xd, w1d, b1d = x.to(dev()), w1.to(dev(), dtype), b1.to(dev())
    zeros, ones = torch.zeros(C, device=dev()), torch.ones(C, device=dev())
    res = torch.zeros((M, C), dtype=dtype, device=dev())
    delta, fails = None, []
    for k in range(4):
        w2 = torch.zeros(C, 4 * C)
        w2[:, k * C:(k + 1) * C] = torch.eye(C)
        w2d = w2.to(dev())
        out = torch.full((M + 8, C), SENT, dtype=dtype, device=dev())
        kutil.call("gcv_k_fused_mlp", _lib.dtype_code(dtype), C, ptr(xd), ptr(w1d), ptr(b1d), ptr(w2d), ptr(zeros), ptr(ones),
                   ptr(res), ptr(out), M)
        o = out.cpu()
        assert (o[M:].float() == SENT).all(), "rows past M were written"
        pre = x.float() + b1[k * C:(k + 1) * C]
        if offgrid or delta is None:                                 # on-grid: the four chunks see the same pre-activations
            delta = _delta(pre, vals.numel(), dtype, offgrid)
        try:
            _judge_gelu(dt, offgrid, o[:M], pre, f"mlp {name} chunk {k}", delta)
        except AssertionError as e:
            fails.append(str(e))
    assert not fails, "; ".join(fails)


# ============================================================================= B. LayerNorm conditioning
FAMILIES = [("offset", R) for R in nu.OFFSETS] + [("scale", 2.0 ** -12), ("scale", 2.0 ** 12), ("const", 1.0), ("const", 100.0)]


def _lnwb(C):
    return rnd((C,), 4, 0.5) + 1.0, rnd((C,), 5, 0.1)


def _row_std(rows):
    """the typical (median) std over the channels of a row"""
    return rows.double().reshape(-1, rows.shape[-1]).std(-1, unbiased=False).median().item()


def _judge_ln(dt, fam, val, got, rows, lw, lb, eps, what, post=lambda z: z):
    """got: the kernel's output (CPU); rows: the float64 pre-LayerNorm rows; post: LayerNorm'd rows -> got's layout.
    Returns None or the failure message; prints the measured line either way."""
    dtype = DTYPES[dt]
    want = post(nu.ln_ref(rows, lw, lb, eps))
    got = got.double()
    err = (got - want).abs().max().item() if torch.isfinite(got).all() else float("inf")
    if fam == "const":
        bound = nu.ln_const_bound(dtype, val, lw.abs().max().item(), eps)
        ratio = "const"
    else:
        e_t = nu.ln_torch_f32_err(rows, lw, lb, eps, nu.ln_ref(rows, lw, lb, eps)) if (fam == "offset" and val > 32) else 0.0
        bound = nu.ln_offset_bound(dtype, val if fam == "offset" else 0, e_t)
        lo, hi = nu.mean_over_std(rows)
        ratio = f"|mean|/std {lo:.3g}..{hi:.3g}"
    print(f"NUMERICS ln {what} {dt} {fam} {val:g}: {ratio} err {err:.3e} bound {bound:.3e}")
    return None if err <= bound else f"{fam} {val:g}: err {err:.3e} > {bound:.3e}"


def _run_families(dt, what, run, x_fed=False):
    """run(fam, val) -> (got, rows, lw, lb, eps[, post]), the arguments of _judge_ln; every family is run and the failures are
    reported together.  x_fed: the offset travels through the 16-bit input itself, so bf16 stops at 128 (the noise must
    survive the rounding of x)"""
    fails = []
    for fam, val in FAMILIES:
        if x_fed and dt == "bf16" and fam == "offset" and val > 128:
            continue
        r = run(fam, val)
        msg = _judge_ln(dt, fam, val, *r[:5], what=what, **({"post": r[5]} if len(r) > 5 else {}))
        if msg:
            fails.append(msg)
    assert not fails, f"{what} {dt}: " + "; ".join(fails)


def _fam_x(fam, val, shape, dtype, seed=1):
    """input of the kernels whose LayerNorm rows ARE the input (rounded to the storage dtype): U(-2, 2) noise, plus the offset
    in units of its std, times the scale, or the constant"""
    if fam == "const":
        return torch.full(shape, val)
    x = rnd(shape, seed, 2.0)
    if fam == "offset":
        x = x + val * (2.0 / math.sqrt(3.0))
    if fam == "scale":
        x = x * val
    return q(x, dtype)


_DW_KINDS = ["tile", "tiny", "tiny_pair", "roll", "mfma", "pair"]      # gcv_dw_plan's kind codes
# (kind, dtypes, (C, H, W, n) from tests/dwcases.py, distinct images): the Mfma launch needs 717 images to be planned as Mfma;
# they repeat three distinct ones, so the float64 reference is computed for three
_DW_SITES = [("roll", ALL, (96, 5, 56, 2), 2), ("mfma", H16, (96, 5, 56, 717), 3), ("pair", ALL, (192, 30, 56, 2), 2),
             ("tiny", ALL, (768, 3, 3, 3), 3), ("tiny_pair", ALL, (1536, 2, 2, 3), 3), ("tile", ALL, (96, 5, 5, 3), 3)]


@pytest.mark.parametrize("site,dt", [(s, dt) for s in _DW_SITES for dt in s[1]], ids=lambda v: v if isinstance(v, str) else v[0])
def test_layernorm_conditioning_dwconv7_ln(site, dt):
    """gcv_k_dwconv7_ln, one shape per kernel kind.  The offset is R times the conv output's row std, injected through the fp32
    conv bias; scale: x and the bias times 2^-12 / 2^12; constant: taps 0 and bias m."""
    kind, _, (C, H, W, n), nd = site
    dtype = DTYPES[dt]
    plan = (ctypes.c_int * 5)()
    assert _lib.load().gcv_dw_plan(_lib.dtype_code(dtype), n, H, W, C, 1, plan) == 0 and _DW_KINDS[plan[0]] == kind
    w = rnd((C, 1, 7, 7), 2, 0.25)
    b0 = rnd((C,), 3, 0.1)
    lw, lb = _lnwb(C)
    convs = {}

    def conv(scale):                                                 # float64 conv of the (rounded) scaled input, no bias
        if scale not in convs:
            x = q(rnd((nd, C, H, W), 1, 2.0) * scale, dtype)
            convs[scale] = (x, F.conv2d(x.double(), w.double(), None, padding=3, groups=C).permute(0, 2, 3, 1))
        return convs[scale]

    std0 = _row_std(conv(1.0)[1] + b0.double())

    def run(fam, val):
        scale = val if fam == "scale" else 1.0
        x, y = conv(scale)
        wk, b = w, b0 * scale
        if fam == "offset":
            b = b0 + val * std0
        if fam == "const":
            wk, b, y = torch.zeros_like(w), torch.full((C,), val), torch.zeros_like(y)
        b = b.float()
        rows = (y + b.double()).repeat(n // nd, 1, 1, 1)
        xd = x.permute(0, 2, 3, 1).repeat(n // nd, 1, 1, 1).contiguous().to(dev(), dtype)
        img = H * W * C
        ybuf = torch.full(((n + 1) * img,), SENT, dtype=dtype, device=dev())
        wd, bd, lwd, lbd = (t.to(dev()) for t in (wk.reshape(C, 49).t().contiguous(), b, lw, lb))
        kutil.call("gcv_k_dwconv7_ln", _lib.dtype_code(dtype), ptr(xd), ptr(wd), ptr(bd), ptr(lwd), ptr(lbd), ptr(ybuf),
                   n, H, W, C, 1e-6)
        out = ybuf.cpu()
        assert (out[n * img:].float() == SENT).all(), "written behind the n images"
        return out[:n * img].reshape(n, H, W, C), rows, lw, lb, 1e-6

    _run_families(dt, f"dwconv7_ln {kind}", run)


@pytest.mark.parametrize("dt", H16)
@pytest.mark.parametrize("C,seg", [(96, (22, 56, 56)), (192, (3, 28, 28))])
def test_layernorm_conditioning_fused_mlp_lnp(dt, C, seg):
    """gcv_k_fused_mlp_lnp (fused_mlp_res_kernel<T, true> at C = 96, xs_mlp_kernel<T, 192, true>): LayerNorm2d + patchify of
    y = resid + gamma (fc2 h + b2) in the MLP kernel's epilogue.  gamma = 1 and the offset in b2 (fp32); scale: resid (rounded
    again) and gamma times 2^-12 / 2^12; constant: fc2 = 0, resid = 0, b2 = m."""
    dtype = DTYPES[dt]
    n, H, W = seg
    M = n * H * W
    x = q(rnd((M, C), 1, 1.5), dtype)
    w1 = q(rnd((4 * C, C), 2, 1 / math.sqrt(C)), dtype)
    w2 = q(rnd((C, 4 * C), 3, 1 / math.sqrt(4 * C)), dtype)
    b1, b2 = rnd((4 * C,), 4, 0.1), rnd((C,), 5, 0.1)
    res0 = rnd((M, C), 7)
    lw, lb = rnd((C,), 8, 0.5) + 1.0, rnd((C,), 9, 0.1)
    # the hidden activation, which the kernel stores in T (its GELU is the subject of the sweeps above)
    h = nu.gelu_ref(x.double() @ w1.double().t() + b1.double()).to(dtype).double()
    hw2 = h @ w2.double().t()
    std0 = _row_std(q(res0, dtype).double() + hw2 + b2.double())
    arr = lambda v: (ctypes.c_int * 4)(v, 0, 0, 0)
    xd, w1d, b1d = x.to(dev(), dtype), w1.to(dev(), dtype), b1.to(dev())
    lwd, lbd = lw.to(dev()), lb.to(dev())

    def post(z):
        return z.reshape(n, H // 2, 2, W // 2, 2, C).permute(0, 1, 3, 2, 4, 5).reshape(M // 4, 4 * C)

    def run(fam, val):
        s = val if fam == "scale" else 1.0
        res, w2k, b, gamma = q(res0 * s, dtype), w2, b2, torch.full((C,), s)
        if fam == "offset":
            b = (b2 + val * std0).float()
        if fam == "const":
            res, w2k, b = torch.zeros(M, C), torch.zeros_like(w2), torch.full((C,), val)
        rows = res.double() + gamma.double() * ((hw2 if fam != "const" else 0.0) + b.double())
        out = torch.full((M // 4 + 3, 4 * C), SENT, dtype=dtype, device=dev())
        w2d, bd, gd, resd = w2k.to(dev()), b.to(dev()), gamma.to(dev()), res.to(dev(), dtype)
        kutil.call("gcv_k_fused_mlp_lnp", _lib.dtype_code(dtype), C, ptr(xd), ptr(w1d), ptr(b1d), ptr(w2d),
                   ptr(bd), ptr(gd), ptr(resd), ptr(lwd), ptr(lbd), 1e-6, 1, arr(0),
                   arr(H * W), arr(W), arr(0), ptr(out), M)
        o = out.cpu()
        assert (o[M // 4:].float() == SENT).all(), "rows behind the last patch row were written"
        return o[:M // 4], rows, lw, lb, 1e-6, post

    _run_families(dt, f"fused_mlp_lnp C={C}", run)


@pytest.mark.parametrize("dt", ALL)
@pytest.mark.parametrize("C", [96, 192])
def test_layernorm_conditioning_stem(dt, C):
    """gcv_k_stem_ln (C = 96) / gcv_k_stem_ln_c: 4x4 stride-4 conv + LayerNorm; offset through the fp32 conv bias, scale
    through x and the bias, constant: weights 0 and bias m.  res 20: 25 tokens per image, a ragged token tile."""
    dtype = DTYPES[dt]
    n, res = 2, 20
    w = q(rnd((C, 3, 4, 4), 2, 0.2), dtype)
    b0 = rnd((C,), 3, 0.1)
    lw, lb = _lnwb(C)
    T = res // 4
    x1 = q(rnd((n, 3, res, res), 1, 2.0), dtype)
    std0 = _row_std(F.conv2d(x1.double(), w.double(), b0.double(), stride=4).permute(0, 2, 3, 1))

    def run(fam, val):
        s = val if fam == "scale" else 1.0
        x = q(rnd((n, 3, res, res), 1, 2.0) * s, dtype)
        wk, b = w, b0 * s
        if fam == "offset":
            b = b0 + val * std0
        if fam == "const":
            wk, b = torch.zeros_like(w), torch.full((C,), val)
        b = b.float()
        rows = F.conv2d(x.double(), wk.double(), b.double(), stride=4).permute(0, 2, 3, 1)
        out = torch.full((n + 1, T, T, C), SENT, dtype=dtype, device=dev())
        xd = x.to(dev(), dtype)
        wd, bd, lwd, lbd = (t.to(dev()) for t in (wk.reshape(C, 48).t().contiguous(), b, lw, lb))
        args = (_lib.dtype_code(dtype), ptr(xd), 3 * res * res, res * res, res, 1, ptr(wd), ptr(bd), ptr(lwd), ptr(lbd),
                ptr(out), n, T, T)
        if C == 96:
            kutil.call("gcv_k_stem_ln", *args, 1e-6)
        else:
            kutil.call("gcv_k_stem_ln_c", *args, C, 1e-6)
        o = out.cpu()
        assert (o[n].float() == SENT).all(), "written behind the n images"
        return o[:n], rows, lw, lb, 1e-6

    _run_families(dt, f"stem_ln C={C}", run)


@pytest.mark.parametrize("dt", ALL)
@pytest.mark.parametrize("C,H,W", [(96, 10, 10), (768, 5, 8)])      # the vectorised kernel (16-bit) and the generic one
def test_layernorm_conditioning_ln_patchify(dt, C, H, W):
    dtype = DTYPES[dt]
    n, Ho, Wo = 2, H // 2, W // 2
    lw, lb = _lnwb(C)

    def post(z):
        z = z[:, :2 * Ho, :2 * Wo]
        return z.reshape(n, Ho, 2, Wo, 2, C).permute(0, 1, 3, 2, 4, 5).reshape(n, Ho, Wo, 4 * C)

    def run(fam, val):
        x = _fam_x(fam, val, (n, H, W, C), dtype)
        out = torch.full((n + 1, Ho, Wo, 4 * C), SENT, dtype=dtype, device=dev())
        xd, lwd, lbd = x.to(dev(), dtype), lw.to(dev()), lb.to(dev())
        kutil.call("gcv_k_ln_patchify", _lib.dtype_code(dtype), ptr(xd), ptr(lwd), ptr(lbd),
                   ptr(out), n, H, W, C, 1e-6)
        o = out.cpu()
        assert (o[n].float() == SENT).all(), "written behind the n images"
        return o[:n], x.double(), lw, lb, 1e-6, post

    _run_families(dt, f"ln_patchify C={C}", run, x_fed=True)


@pytest.mark.parametrize("dt", ALL)
def test_layernorm_conditioning_layernorm_rows(dt):
    dtype = DTYPES[dt]
    rows_n, C = 37, 384
    lw, lb = _lnwb(C)

    def run(fam, val):
        x = _fam_x(fam, val, (rows_n, C), dtype)
        out = torch.full((rows_n + 2, C), SENT, dtype=dtype, device=dev())
        xd, lwd, lbd = x.to(dev(), dtype), lw.to(dev()), lb.to(dev())
        kutil.call("gcv_k_layernorm_rows", _lib.dtype_code(dtype), ptr(xd), ptr(lwd), ptr(lbd),
                   ptr(out), rows_n, C, 1e-5)
        o = out.cpu()
        assert (o[rows_n:].float() == SENT).all(), "rows past the last were written"
        return o[:rows_n], x.double(), lw, lb, 1e-5

    _run_families(dt, "layernorm_rows", run, x_fed=True)


@pytest.mark.parametrize("dt", ALL)
def test_layernorm_conditioning_pool_ln(dt):
    """gcv_k_pool_ln: mean over the tokens, then LayerNorm.  The rows are the float64 token means of the rounded input."""
    dtype = DTYPES[dt]
    n, HW, C = 5, 9, 768
    lw, lb = _lnwb(C)

    def run(fam, val):
        x = _fam_x(fam, val, (n, HW, C), dtype)
        out = torch.full((n + 2, C), SENT, dtype=dtype, device=dev())
        xd, lwd, lbd = x.to(dev(), dtype), lw.to(dev()), lb.to(dev())
        kutil.call("gcv_k_pool_ln", _lib.dtype_code(dtype), ptr(xd), ptr(lwd), ptr(lbd),
                   ptr(out), n, HW, C, 1e-6)
        o = out.cpu()
        assert (o[n:].float() == SENT).all(), "rows past the last were written"
        return o[:n], x.double().mean(1), lw, lb, 1e-6

    _run_families(dt, "pool_ln", run, x_fed=True)


@pytest.mark.parametrize("dt", ALL)
def test_layernorm_conditioning_patch_merge_ln(dt):
    """gcv_k_patch_merge_ln: Swin's 2x2 patch merging, LayerNorm over the 4 C gathered channels"""
    dtype = DTYPES[dt]
    n, H, C = 2, 6, 96
    lw, lb = _lnwb(4 * C)

    def run(fam, val):
        x = _fam_x(fam, val, (n, H, H, C), dtype)
        rows = torch.cat([x[:, 0::2, 0::2], x[:, 1::2, 0::2], x[:, 0::2, 1::2], x[:, 1::2, 1::2]], -1).double()
        out = torch.full((n + 1, H // 2, H // 2, 4 * C), SENT, dtype=dtype, device=dev())
        xd, lwd, lbd = x.to(dev(), dtype), lw.to(dev()), lb.to(dev())
        kutil.call("gcv_k_patch_merge_ln", _lib.dtype_code(dtype), ptr(xd), ptr(lwd), ptr(lbd),
                   ptr(out), n, H, H, C, 1e-5)
        o = out.cpu()
        assert (o[n].float() == SENT).all(), "written behind the n images"
        return o[:n], rows, lw, lb, 1e-5

    _run_families(dt, "patch_merge_ln", run, x_fed=True)


# ============================================================================= C. Softmax of the Swin window attention
_ATTN = (2, 14, 21, 96, 3, 3)
# fp32 storage runs swin_window_attn_kernel; 16-bit storage swin_window_attn_mfma_kernel, and swin_window_attn_kernel<T> when
# qkv starts one element into its allocation (tests/test_kernels_gpu.py, swin_attn_case)
_ATTN_SITES = [("f32", "valu"), ("bf16", "mfma"), ("bf16", "valu"), ("f16", "mfma"), ("f16", "valu")]


@pytest.mark.parametrize("dt,kernel", _ATTN_SITES)
@pytest.mark.parametrize("variant", ["uniform", "wide", "mask100"])
def test_softmax_off_distribution_swin_window_attn(variant, dt, kernel):
    """gcv_k_swin_window_attn at (B, H, W, C, nH, shift) = (2, 14, 21, 96, 3, 3) on the inputs of kcases.swin_attn's variants,
    with the family's comparator against float64, sentinels around the result, and a finite result required:
      uniform   q = 0 and a zero table: every row is the plain mean of its region's V rows; a padded key counted in the
                sum shows at its largest
      wide      logits from -136 to 136 in every row, the maximum on the upper lane half of the MFMA kernel (key index bit 2)
                for the even queries and on the lower for the odd: a maximum taken per half, or none subtracted (inf / nan)
      mask100   the last key of each window leads the others by 120: masked by -100 it still carries the row, where a kernel
                that masks with -inf returns the softmax of the in-region keys
    tests/test_numerics_cpu.py checks those properties of the inputs and that the comparator rejects each defect."""
    from tests.test_kernels_gpu import swin_attn_case
    dtype = DTYPES[dt]
    swin_attn_case(dtype, *_ATTN, kernel, qkv_off=1 if (kernel == "valu" and dt != "f32") else 0, variant=variant)
