"""Numerics helpers of tests/test_numerics_gpu.py and tests/test_numerics_cpu.py: value sets off the U(-1, 1) distribution of
kutil.rnd, float64 references, CPU restatements of two device formulas (the packed-fp16 GELU polynomial of csrc/gemm.h GeluH16
and the one-pass LayerNorm statistics that are the first pass of the 16-bit hot-path kernels), and the bound functions
both test files apply.  Nothing here needs a GPU."""
import math

import numpy as np
import torch
import torch.nn.functional as F

from tests import kutil

_FMT = {torch.float16: (10, -14), torch.bfloat16: (7, -126), torch.float32: (23, -126)}     # mantissa bits, minimum exponent


# ----------------------------------------------------------------------------- value sets
def finite_grid(dtype):
    """every finite value of a 16-bit dtype, as a tensor of that dtype (63 488 for fp16, 65 280 for bf16; both zeros)"""
    inf_bits = {torch.float16: 0x7C00, torch.bfloat16: 0x7F80}[dtype]
    pos = np.arange(0, inf_bits, dtype=np.uint16)
    bits = np.concatenate([pos, pos | np.uint16(0x8000)])
    return torch.from_numpy(bits.view(np.int16).copy()).view(dtype)


def shuffled(v, seed=7):
    """seeded permutation of a 1-D value set: in grid order the two values of a packed pair (and the rows of an MFMA block)
    are neighbours on the grid, and a kernel that mixed them up would go unnoticed"""
    return v[torch.randperm(v.numel(), generator=torch.Generator().manual_seed(seed))]


def offgrid_bias(n, seed=11):
    """fp32 U(-2^-6, 2^-6): not representable in a 16-bit type (24 random mantissa bits)"""
    return kutil.rnd((n,), seed, 2.0 ** -6)


def tile_to(v, count):
    """the 1-D value set repeated (and cut) to `count` elements"""
    reps = -(-count // v.numel())
    return v.repeat(reps)[:count]


# ----------------------------------------------------------------------------- GELU
def gelu_ref(x):
    """exact GELU in float64 as 0.5 x erfc(-x / sqrt 2): 1 + erf would lose the negative tail to cancellation"""
    x = x.double()
    return 0.5 * x * torch.special.erfc(-x / math.sqrt(2.0))


def ulp(v, dtype):
    """spacing of `dtype` at |v| (float64 tensor in, float64 out; the subnormal spacing below the smallest normal)"""
    mant, emin = _FMT[dtype]
    _, e = torch.frexp(v.double().abs())           # |v| = m 2^e, m in [0.5, 1): floor(log2 |v|) = e - 1 (e = 0 for v = 0)
    e = torch.where(v == 0, torch.full_like(e, emin), e - 1).clamp(min=emin)
    return torch.ldexp(torch.ones_like(v, dtype=torch.float64), e - mant)


# the coefficients of csrc/gemm.h GeluH16::kC before the factor -0.5 (h(a) = a/2 erfc(a / sqrt 2) in t = a/2 - 1, degree 8)
GELU_H16_COEF = (4.543376254e-02, -1.712937983e-01, 2.188785784e-01, 1.159314756e-02, -3.094936844e-01, 2.450228537e-01,
                 3.058419957e-02, -8.537015778e-02, 1.466048626e-02)


def _fma16(a, b, c):
    """fp16 fma with one rounding: the product of two fp16 values and its sum with a third are exact in float64 here
    (|values| <= 4, quantum >= 2^-48), and numpy rounds float64 -> float16 directly"""
    return (a.astype(np.float64) * b.astype(np.float64) + c.astype(np.float64)).astype(np.float16)


def gelu_h16_ref(pre, dtype, coef=GELU_H16_COEF, clamp=4.0, swap_pairs=False, packed_finish=True):
    """CPU restatement of GeluH16 (csrc/gemm.h): `pre` fp32 pre-activations -> the stored T value, as float64.  Same
    coefficients (each times -0.5, rounded to fp16), the clamp of |x| at 4, fp16 Horner with single-rounding fma, and the two
    last steps: fp16 storage y = fma16(p, 2, max(fp16(x), 0)) (finish_pk), bf16 storage y = bf16(fp32 fma(p, 2, max(x, 0))).
    finish_pk is the last step of the sites that build MFMA fragments (gelu_h16_frag / finish_frag: fused_mlp_res_kernel,
    xs_mlp_kernel, xs_pw1_kernel).  The sites behind act4n -> gelu_h16_n (the tile GEMM, the LDS-DMA GEMM and
    fused_mlp_kernel<T, 96, 4>) end in the fp32 `finish` for fp16 storage as well and round the result to fp16 when they
    store it: packed_finish = False restates those.  The GPU tests take delta from the default for every site, as the bound
    is defined; on off-grid fp16 inputs the two forms differ by a few 1e-6 in their excess, inside delta's quarter.
    The keyword arguments are the defects tests/test_numerics_cpu.py plants: other coefficients, another clamp, and
    swap_pairs = True hands each value the polynomial of its pair partner (values 2c and 2c + 1 share a packed register)."""
    assert dtype in (torch.float16, torch.bfloat16)
    x = pre.detach().float().reshape(-1).numpy()
    with np.errstate(over="ignore"):
        xh = x.astype(np.float16)                                      # v_cvt_pk_f16_f32: round to nearest even, inf beyond 65 504
    k = [np.float16(np.float32(-0.5) * np.float32(c)) for c in coef]
    a = np.minimum(np.abs(xh), np.float16(clamp))
    t = _fma16(a, np.float16(0.5), np.float16(-1.0))
    p = _fma16(np.full_like(t, k[8]), t, np.full_like(t, k[7]))
    for j in range(6, -1, -1):
        p = _fma16(p, t, np.full_like(t, k[j]))
    if swap_pairs:
        assert p.size % 2 == 0
        p = p.reshape(-1, 2)[:, ::-1].reshape(-1)
    if dtype == torch.float16 and packed_finish:
        with np.errstate(over="ignore", invalid="ignore"):
            y = _fma16(p, np.full_like(p, np.float16(2.0)), np.maximum(xh, np.float16(0.0)))
        out = torch.from_numpy(y.astype(np.float64))
    else:
        y32 = (p.astype(np.float64) * 2.0 + np.maximum(x, np.float32(0.0)).astype(np.float64)).astype(np.float32)
        out = torch.from_numpy(y32).to(dtype).double()
    return out.reshape(pre.shape)


def gelu_f32_bound(pre, want):
    """fp32 storage: erf_fast's 6e-7 (csrc/gemm.h) through 0.5 x (1 + erf), plus the roundings of the product"""
    return 6e-7 * pre.double().abs() + 2.0 ** -22 * want.abs()


def gelu_round_term(pre, want, dtype, offgrid):
    """the part of a 16-bit site's error that is rounding by design: half a step of T at the result, and for fp16 storage of
    off-grid pre-activations half a step of fp16 at x (finish_pk rounds x to fp16 before the ReLU part)"""
    r = 0.5 * ulp(want, dtype)
    if offgrid and dtype == torch.float16:
        r = r + 0.5 * ulp(pre.double(), torch.float16)
    return r


def gelu_excess(got, pre, dtype, offgrid):
    """largest |got - exact| beyond the rounding term over a value set (may be negative); got float64"""
    want = gelu_ref(pre)
    return ((got.double() - want).abs() - gelu_round_term(pre, want, dtype, offgrid)).max().item()


def gelu_delta(pre, dtype, offgrid):
    """the polynomial allowance of a value set: 1.25 x the restatement's own largest excess over the rounding term (the
    quarter covers denormal handling and fma contraction differences between the emulation and the packed pipe)"""
    return 1.25 * gelu_excess(gelu_h16_ref(pre, dtype), pre, dtype, offgrid)


def gelu_h16_holds(got, pre, dtype, offgrid, delta):
    """(bound holds, measured excess) of a 16-bit GELU site on one value set"""
    ex = gelu_excess(got, pre, dtype, offgrid)
    return ex <= delta, ex


# ----------------------------------------------------------------------------- LayerNorm
def ln_ref(rows, w, b, eps):
    """float64 LayerNorm over the last dimension"""
    r = rows.double()
    mean = r.mean(-1, keepdim=True)
    var = ((r - mean) ** 2).mean(-1, keepdim=True)
    return (r - mean) / torch.sqrt(var + eps) * w.double() + b.double()


def mean_over_std(rows):
    """(min, max) of |mean| / std over the rows of a float64 tensor (inf where a row is constant)"""
    r = rows.double().reshape(-1, rows.shape[-1])
    ratio = r.mean(-1).abs() / r.std(-1, unbiased=False)
    return ratio.min().item(), ratio.max().item()


def ln_onepass_ref(rows, w, b, eps):
    """float32 restatement of one-pass LayerNorm statistics, sums taken sequentially over the channels (the worst order):
    rstd = 1 / sqrt(max(E[x^2] - mean^2, 0) + eps), out = (x rstd - mean rstd) w + b.  float64 out."""
    v = rows.float().reshape(-1, rows.shape[-1])
    C = v.shape[1]
    s, q = torch.zeros(v.shape[0]), torch.zeros(v.shape[0])
    for c in range(C):
        s = s + v[:, c]
        q = torch.addcmul(q.double(), v[:, c].double(), v[:, c].double()).float()      # fmaf
    mean, ex2 = s * (1.0 / C), q * (1.0 / C)
    var = (ex2.double() - mean.double() * mean.double()).float().clamp(min=0.0)        # fmaf(-mean, mean, ex2)
    rstd = 1.0 / torch.sqrt(var + eps)
    nmr = -mean * rstd
    z = (v.double() * rstd[:, None].double() + nmr[:, None].double()).float()
    return (z * w.float() + b.float()).double().reshape(rows.shape)


def ln_twopass_ref(rows, w, b, eps):
    """float32 restatement of centred statistics (sequential mean, then sequential centred squares); float64 out"""
    v = rows.float().reshape(-1, rows.shape[-1])
    C = v.shape[1]
    s = torch.zeros(v.shape[0])
    for c in range(C):
        s = s + v[:, c]
    mean = s * (1.0 / C)
    d = v - mean[:, None]
    q = torch.zeros(v.shape[0])
    for c in range(C):
        q = torch.addcmul(q.double(), d[:, c].double(), d[:, c].double()).float()
    rstd = 1.0 / torch.sqrt(q * (1.0 / C) + eps)
    return ((d * rstd[:, None]) * w.float() + b.float()).double().reshape(rows.shape)


def ln_torch_f32_err(rows, w, b, eps, want):
    """e_torch: max |F.layer_norm in float32 - float64 reference| on the same rows rounded to fp32"""
    got = F.layer_norm(rows.float(), (rows.shape[-1],), w.float(), b.float(), eps)
    return (got.double() - want).abs().max().item()


OFFSETS = (0, 8, 32, 128, 1000)      # |mean| / std of the offset family


def ln_base_bound(dtype):
    """B: the bound of the LayerNorm tests of tests/test_kernels_gpu.py"""
    return kutil.tol(dtype, 3.0)


def ln_offset_bound(dtype, R, e_torch):
    """offset family: B up to |mean| / std = 32; beyond, B + 4 e_torch (4: another summation order than torch's)"""
    return ln_base_bound(dtype) + (4.0 * e_torch if R > 32 else 0.0)


def ln_const_bound(dtype, m, lnw_max, eps):
    """constant rows against ln_b: B + 4 x 2^-24 |m| max|ln_w| / sqrt(eps) — two roundings of the mean (with a factor 2 for
    the order they are taken in), amplified by rstd <= 1 / sqrt(eps)"""
    return ln_base_bound(dtype) + 4.0 * 2.0 ** -24 * abs(m) * lnw_max / math.sqrt(eps)


def offset_rows(nrows, C, R, seed=21):
    """rows R * std + U(-1, 1), std that of U(-1, 1) (the model of the issue's table); fp32"""
    return kutil.rnd((nrows, C), seed) + R * (1.0 / math.sqrt(3.0))
