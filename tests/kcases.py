"""One builder per kernel family whose output feeds the verdict: the CPU inputs of a case exactly as the GPU test uploads
them, the float64 reference, the comparator, an honest float32 model, and the family's planted defects.  The GPU tests
(tests/test_kernels_gpu.py, tests/test_mlp_bias_init_gpu.py, the softmax cases of tests/test_numerics_gpu.py) and the CPU
audit (tests/test_kernel_sensitivity_cpu.py) share them, so what the audit proves about the comparator and the inputs
holds for what the GPU tests assert.  The Swin-T kernels (row A6) are here too, though the verdict does not pass through
them.  The ten Grad-CAM backward kernels have their builders in tests/camcases.py, on the Case / MultiCase of this module and
with their e in E below (their GPU tests: tests/test_cam_kernels_gpu.py).  Nothing here needs a GPU.

A builder returns a Case:
  inputs            name -> CPU tensor (fp32 holding values of the storage dtype where the kernel reads that dtype)
  ref(inputs)       the plain reference in float64 on those inputs.  Where the kernel rounds the hidden activation to the
                    storage dtype (the fused MLPs), the reference rounds it too.
  check(got, want, inputs) -> (ok, message)
  defects           name -> function(inputs) -> float64 result of a reference with that defect planted
  model(inputs)     an honest float32 implementation (torch matmul / conv in float32, the 16-bit GELU through
                    numutil.gelu_h16_ref), rounded to the storage dtype: what a correct kernel may legitimately return

Comparator.  16-bit storage, per element: |got - want| <= 0.5 ulp_T(want) + e, e one scalar per (family, dtype) in E
below: fp32 accumulation order, hidden values that land on the other side of a rounding step, the packed GELU polynomial.
Its largest per-element bound must stay <= kutil.tol(dtype, scale) of the test it replaces (asserted on every call), so
nothing gets weaker.  fp32 storage, and the fp32 partial sums of split-K, keep their flat bound.

Inputs.  Every vector term (bias, b1, b2, gamma, LayerNorm weight / bias, the 49 depthwise taps) is drawn from +-[lo, hi],
never U(-s, s): an element that is dropped, rotated in from its neighbour or swapped moves the output by at least lo times
its factor.  The shortcut of the residual families is |res| <= 0.25 so that the output's rounding step stays below the
branch's smallest term.

Defects that do not apply to a family (every other entry of the catalogue applies):
  split-K          no bias, gamma, activation or shortcut: contraction and row defects only (plus a K index at a split edge,
                   where there is one: the backward contractions' launch is one split of the whole K)
  GEMM bias/act    no gamma, no shortcut, no branch to scale; ReLU-for-LeakyReLU only where the activation is LeakyReLU;
                   activation-omitted only where there is one
  POOL4 / CONVT    no gamma, no shortcut; CONVT has no pool, POOL4's activation is ReLU
  dw7x7 + LN       no gamma, no shortcut, no activation; its contraction is the 49 taps (one tap zeroed on one channel); the two
                   band-seam defects (a band's first rows without the input rows above it, its last row from the row before)
                   need a band kernel with more than one band per image
  fused MLP        no pool, no taps; LN-patchify row defects exist only behind gcv_k_fused_mlp_lnp, and the
                   previous-segment-geometry defect needs a second segment
  M = 1            no row before the last one: the row defects are left out at a single row
  stem             its contraction is the patch's 48 values (w[:, k] zeroed, kx / ky transposed); no activation, no shortcut
  LN-patchify      no contraction, no bias in front of the LayerNorm; the kept last column needs an odd W and a second patch
                   row (with one, every such write lands behind the output, where the GPU test keeps a sentinel)
  pool + LN        no contraction; the token left out of the mean needs HW > 1, the row order a mapping (seg_n > 0)
  first conv       stride 2 at even H, W reads no padding on the right or below: its clamped edges are the left and the top
                   ones; pool-over-three only with the pool, ReLU-for-LeakyReLU only without
  last convT       contraction defects are whole input channels (the weights stay fp32: no K tile)
  reparam          no activation; a slab, the bias, the exponent, eps' row and the two orders z could be left in
  head tail        no b1, slab or activation without the split-K reduce in front
  resize + MSE     no vector term: coordinates, clamps, lerp weights, channel and axis order, and the two MSE reductions
  window attention no bias vector, gamma, activation or shortcut; its table, index, scale, mask, roll, window and key-order
                   defects are its own (swin_attn).  Mask and roll defects need a shift, the H-for-W and nWy-for-nWx ones
                   H != W, the next head's column a second head, the window before a second window, the image before a second
                   image; table rows 0 and 168 need a window that the mask does not split
  patch merging    no contraction, no bias in front of the LayerNorm; rows strided by H need H != W
  token mean       no vector term; the token left out needs L > 1, the image before n > 1, the unwritten last channel a
                   partly filled 256-column trip (C % 256 != 0)
  layernorm_rows   no contraction; the padded-width statistics and the padded lanes in the variance need C % 64 != 0
A family with several outputs (reparam, resize + MSE) is a MultiCase: one comparator per output, a defect counts as rejected
when any of them rejects it.
Where a defect names "one" element, it is the vector's last element, the pair (2c, 2c + 1) at c = n // 4, the centre tap of
the last channel, hidden unit 4C - 31, and for an omitted activation the column with the lowest bias (behind the 2x2 pool
an omitted ReLU shows only where all four pixels of a window are negative).
The erf-versus-tanh GELU and the LayerNorm eps belong to tests/test_numerics_*.
"""
import math

import torch
import torch.nn.functional as F

from tests import kutil, numutil
from tests.kutil import rnd

F16, BF16, F32 = torch.float16, torch.bfloat16, torch.float32
NAMES = {F16: "f16", BF16: "bf16", F32: "f32"}

# e per (family, dtype): 3 x the largest excess |got - want64| - 0.5 ulp_T(want) measured on the MI355X over all of the family's
# cases in the GPU tests (the measured value in the comment).  An fp32 accumulator rounded once to T exceeds half a step by
# at most its own fp32 error, hence the 1e-7s measured for the families without a hidden rounding or a polynomial.  Those
# get the floor FP32_ACC instead of 3 x 1e-7: the honest float32 model of tests/test_kernel_sensitivity_cpu.py sums in the
# host BLAS's order, reaches 3e-7 there already, and must pass on any host; sixteen fp32 roundings at 1.0 is still a
# thousand times below the smallest planted defect.  "gemm_bias_gelu" carries GeluH16's polynomial, the MLP families that
# and the hidden values which land on the other side of a rounding step (the LN-patchify epilogue scales both by
# lw / std of a row, about 4 here).  The small kernels of the verdict path (stem to resize) round an fp32 result once: all
# at the floor but the bf16 stem, whose matrix-pipe LayerNorm reaches 4.3e-7.  Of the Swin-T kernels the three LayerNorm / mean
# families are at the floor too; the window attention carries the probabilities that its matrix-pipe kernel rounds to T.
FP32_ACC = 16 * 2.0 ** -24             # 9.54e-07
E = {
    ("mlp", BF16): 2.4e-3,             # 8.31e-04
    ("mlp", F16): 1.3e-3,              # 4.62e-04
    ("mlp_lnp", BF16): 1.3e-2,         # 4.41e-03
    ("mlp_lnp", F16): 6.6e-3,          # 2.23e-03
    ("gemm_bias_gelu", BF16): 1.7e-3,  # 5.96e-04
    ("gemm_bias_gelu", F16): 1.7e-3,   # 5.89e-04
    ("dw_ln", BF16): 2.4e-6,           # 8.33e-07
    ("dw_ln", F16): 2.7e-6,            # 9.16e-07
    ("gemm_resid", BF16): FP32_ACC,    # 2.33e-07
    ("gemm_resid", F16): 1.0e-6,       # 3.38e-07
    ("gemm_bias_act", BF16): FP32_ACC,   # 1.41e-07
    ("gemm_bias_act", F16): FP32_ACC,    # 1.63e-07
    ("conv_s2", BF16): FP32_ACC,       # 2.17e-08
    ("conv_s2", F16): FP32_ACC,        # 7.64e-08
    ("pool4", BF16): FP32_ACC,         # 3.16e-08
    ("pool4", F16): FP32_ACC,          # 1.31e-07
    ("convt", BF16): FP32_ACC,         # 2.61e-08
    ("convt", F16): FP32_ACC,          # 7.90e-08
    ("stem", BF16): 1.3e-6,            # 4.34e-07
    ("stem", F16): FP32_ACC,           # 2.42e-07
    ("ln_patchify", BF16): FP32_ACC,   # 1.99e-07
    ("ln_patchify", F16): FP32_ACC,    # 2.58e-07
    ("pool_ln", BF16): FP32_ACC,       # 1.11e-08
    ("pool_ln", F16): FP32_ACC,        # 1.56e-08
    ("conv3_first", BF16): FP32_ACC,   # 7.45e-08
    ("conv3_first", F16): FP32_ACC,    # 1.73e-07
    ("convt2_small", BF16): FP32_ACC,  # below 0: never past half a step
    ("convt2_small", F16): FP32_ACC,   # 9.83e-09
    ("reparam", BF16): FP32_ACC,       # 9.36e-09 (z; mu is fp32 with a flat bound)
    ("reparam", F16): FP32_ACC,        # 6.13e-08
    ("resize", BF16): FP32_ACC,        # 0 (recon; msepart and mse are fp32 with a relative bound, MSE_REL)
    ("resize", F16): FP32_ACC,         # 0
    ("swin_attn", BF16): 4.9e-3,       # 1.63e-03 (the MFMA kernel rounds exp(s - max) to T in front of P.V; the off-distribution
    ("swin_attn", F16): 6.6e-4,        # 2.21e-04  softmax cases of tests/test_numerics_gpu.py stay below: 6.0e-04 / 7.0e-05)
    ("patch_merge_ln", BF16): FP32_ACC,  # 1.70e-07
    ("patch_merge_ln", F16): FP32_ACC,   # 1.38e-07
    ("mean_tokens", BF16): FP32_ACC,   # 0
    ("mean_tokens", F16): FP32_ACC,    # 0
    ("layernorm_rows", BF16): FP32_ACC,  # 6.31e-08
    ("layernorm_rows", F16): FP32_ACC,   # 5.97e-08
    # the Grad-CAM backward kernels (tests/camcases.py): fp32 outputs against e s, s the scale of the element or row.  Measured:
    # largest |got - want64| / s over the family's cases, for the T outputs of scale_rows / gelu_bwd the excess over half a step.
    # All at the floor but dw_ln_bwd: its case of a constant depthwise bias 0.25 and a token variance of eps' size holds
    # deviations of 1e-3 on 0.25, where one fp32 rounding of the raw conv output is 3e-5 of the deviation; the other dw_ln_bwd
    # cases stay at 2.2e-07.
    ("head_bwd", F32): FP32_ACC,        # 5.87e-08
    ("head_bwd", BF16): FP32_ACC,       # 6.47e-08
    ("head_bwd", F16): FP32_ACC,        # 7.55e-08
    ("bb_bwd", F32): FP32_ACC,          # 7.05e-08
    ("bb_bwd", BF16): FP32_ACC,         # 7.55e-08
    ("bb_bwd", F16): FP32_ACC,          # 6.37e-08
    ("pool_ln_bwd", F32): FP32_ACC,     # 1.96e-07
    ("pool_ln_bwd", BF16): FP32_ACC,    # 1.65e-07
    ("pool_ln_bwd", F16): FP32_ACC,     # 1.77e-07
    ("cam", F32): FP32_ACC,             # 1.70e-08
    ("cam", BF16): FP32_ACC,            # 1.74e-08
    ("cam", F16): FP32_ACC,             # 1.87e-08
    ("scale_rows", F32): FP32_ACC,      # below 0: never past half a step
    ("scale_rows", BF16): FP32_ACC,     # below 0: never past half a step
    ("scale_rows", F16): FP32_ACC,      # below 0: never past half a step
    ("gelu_bwd", F32): FP32_ACC,        # 3.52e-08
    ("gelu_bwd", BF16): FP32_ACC,       # 9.87e-11
    ("gelu_bwd", F16): FP32_ACC,        # 4.45e-09
    ("dw_ln_bwd", F32): 5.6e-06,        # 1.86e-06
    ("dw_ln_bwd", BF16): 6.0e-06,       # 1.99e-06
    ("dw_ln_bwd", F16): 5.0e-06,        # 1.63e-06
    ("dw_dgrad_res", F32): FP32_ACC,    # 2.89e-07
    ("down_ln_bwd", F32): FP32_ACC,     # 1.98e-07
    ("down_ln_bwd", BF16): FP32_ACC,    # 2.19e-07
    ("down_ln_bwd", F16): FP32_ACC,     # 2.31e-07
    ("cam2", F32): FP32_ACC,            # 1.22e-07
    ("cam2", BF16): FP32_ACC,           # 1.22e-07
    ("cam2", F16): FP32_ACC,            # 1.22e-07
}
SPLITK_BOUND = {F32: 2e-5, BF16: 1e-4, F16: 1e-4}      # fp32 partial sums in every storage dtype: the flat bound as before

_CHUNK = 1 << 23


def q(t, dtype):
    """round a CPU tensor through the storage dtype; fp32 out"""
    return t.to(dtype).float()


def round_to(t64, dtype):
    """a float64 result as the storage dtype would hold it; float64 out.  (torch converts through float32: next to a tie of
    T the result can be the other neighbour, 2^-25 |v| further away than the nearest — a quarter of E's floor at |v| = 8.)"""
    return t64.to(dtype).double()


def signed(shape, seed, lo, hi):
    """uniform in +-[lo, hi].  In a vector, element 2c + 1 takes the sign opposite to element 2c's, so the two values of a
    packed pair differ by at least 2 lo: swapped, each moves by that much."""
    u = rnd(shape, seed)                                   # U(-1, 1): the sign, and |u| for the magnitude
    sign = torch.sign(u + (u == 0).float())
    if len(shape) == 1:
        sign[1::2] = -sign[0:shape[0] - shape[0] % 2:2]
    return sign * (lo + (hi - lo) * u.abs())


def vec_variants(v):
    """the three vector defects: last element zeroed, rotated by one, elements 2c and 2c + 1 swapped (c = n // 4)"""
    n = v.numel()
    z, s = v.clone(), v.clone()
    z[n - 1] = 0
    c = n // 4
    s[2 * c], s[2 * c + 1] = v[2 * c + 1], v[2 * c]
    return {"one_zeroed": z, "rotated": torch.roll(v, 1), "pair_swapped": s}


def k_indices(K):
    """first, last, and one index next to a 32-element K-tile edge"""
    return {"k_first": 0, "k_last": K - 1, "k_tile_edge": 32 if K > 33 else min(31, K - 1)}


def _with(inp, **kw):
    d = dict(inp)
    d.update(kw)
    return d


class Case:
    def __init__(self, family, dtype, inputs, ref, model, defects, scale, flat=None, what="", bound=None):
        self.family, self.dtype, self.inputs, self.ref, self.model, self.defects = family, dtype, inputs, ref, model, defects
        self.what = f"{what or family} {NAMES[dtype]}"
        self.tol_before = kutil.tol(dtype, scale) if flat is None else flat      # the bound of the test this replaces
        self.e = E[(family, dtype)] if (flat is None and dtype != F32) else None
        self.bound = bound               # a float64 bound per element of the result, in place of the flat one (<= flat, asserted)
        self._want = None

    def want(self):
        """ref(inputs), computed once"""
        if self._want is None:
            self._want = self.ref(self.inputs)
        return self._want

    def measure(self, got, want):
        """largest |got - want|, largest err / bound with its flat index, largest excess err - 0.5 ulp_T(want) (the
        quantity E is set from; for a flat bound the largest error itself)"""
        g, w = got.detach().cpu().reshape(-1), want.reshape(-1)
        assert g.numel() == w.numel(), f"{self.what}: {tuple(got.shape)} against {tuple(want.shape)}"
        out = {"err": 0.0, "ratio": 0.0, "at": 0, "excess": -math.inf, "bound": 0.0}
        for s in range(0, g.numel(), _CHUNK):
            wd = w[s:s + _CHUNK].double()
            err = (g[s:s + _CHUNK].double() - wd).abs()
            err = torch.where(torch.isfinite(err), err, torch.full_like(err, math.inf))
            if self.bound is not None:
                bound, ex = self.bound.reshape(-1)[s:s + _CHUNK].double(), err.max().item()
                assert bound.max().item() <= self.tol_before, \
                    f"{self.what}: per-element bound {bound.max().item():.3e} above the flat bound {self.tol_before:.3e}"
            elif self.e is None:
                bound, ex = torch.full_like(err, self.tol_before), err.max().item()
            else:
                half = 0.5 * numutil.ulp(wd, self.dtype)
                bound, ex = half + self.e, (err - half).max().item()
                assert bound.max().item() <= self.tol_before, \
                    f"{self.what}: per-element bound {bound.max().item():.3e} above the flat bound {self.tol_before:.3e}"
            ratio = err / bound
            i = int(ratio.argmax())
            if ratio[i].item() >= out["ratio"]:
                out.update(ratio=ratio[i].item(), at=s + i, bound=bound[i].item())
            out["err"], out["excess"] = max(out["err"], err.max().item()), max(out["excess"], ex)
        return out

    def check(self, got, want, inputs=None):
        m = self.measure(got, want)
        ok = m["ratio"] <= 1.0
        idx = tuple(int(i) for i in torch.unravel_index(torch.tensor(m["at"]), want.shape)) if want.dim() else ()
        msg = (f"{self.what}: max |diff| {m['err']:.3e}, worst err/bound {m['ratio']:.2f} at {idx} (bound there "
               f"{m['bound']:.3e}), excess {m['excess']:.3e}"
               + (f" (e = {self.e:.1e})" if self.e is not None else
                  f" ({'per-element bound, at most' if self.bound is not None else 'flat bound'} {self.tol_before:.1e})"))
        return ok, msg

    def assert_close(self, got):
        ok, msg = self.check(got, self.want(), self.inputs)
        print(msg)
        assert ok, msg

    def to_storage(self, t64):
        """a float64 result as the kernel's output buffer would hold it (fp32 where the bound is flat)"""
        return t64.float() if self.e is None else round_to(t64, self.dtype)


def _act64(v, act, noact_col=None, relu_for_leaky=False):
    """activation of the GEMM epilogues on (..., N) float64: 0 none, 1 ReLU, 2 exact GELU, 3 LeakyReLU(0.01)"""
    if act == 0:
        return v
    if act == 1 or (act == 3 and relu_for_leaky):
        y = v.clamp(min=0)
    elif act == 2:
        y = numutil.gelu_ref(v)
    else:
        y = torch.where(v >= 0, v, 0.01 * v)
    if noact_col is not None:
        y = y.clone()
        y[..., noact_col] = v[..., noact_col]
    return y


def _act32(v, act, dtype):
    """the same in float32 as a kernel computes it: the 16-bit GELU sites behind act4n end in the fp32 finish"""
    if act == 0:
        return v
    if act == 1:
        return v.clamp(min=0)
    if act == 3:
        return torch.where(v >= 0, v, 0.01 * v)
    if dtype == F32:
        return F.gelu(v)
    return numutil.gelu_h16_ref(v, dtype, packed_finish=False).float()


def _d(inp):
    return {k: v.double() for k, v in inp.items()}


# ----------------------------------------------------------------------------- GEMM epilogues on a plain A
def gemm(epi, M, N, K, dtype, act=0, k_per_split=0):
    """epi: "bias_act", "resid" (X + gamma (A W^T + bias), in place) or "splitk" (fp32 partial sums, summed by the test)"""
    inp = {"A": q(rnd((M, K), 1), dtype), "W": q(rnd((N, K), 2, 1 / math.sqrt(K)), dtype)}
    if epi != "splitk":
        inp["bias"] = signed((N,), 3, 0.05, 0.2)
    if epi == "resid":
        inp["gamma"], inp["X"] = signed((N,), 4, 0.25, 0.5), q(rnd((M, N), 5, 0.25), dtype)

    def ref(i, branch=1.0, gamma_one=False, noact_col=None, relu_for_leaky=False, last_from_prev=False, resid_shift=False):
        i = _d(i)
        pre = i["A"] @ i["W"].t()
        if epi == "splitk":
            y = pre
        else:
            y = _act64(pre + i["bias"], act, noact_col, relu_for_leaky)
        if last_from_prev:
            y = y.clone()
            y[M - 1] = y[M - 2]
        if epi == "resid":
            X = i["X"]
            if resid_shift:
                X = X.clone()
                X[M - 1] = X[M - 2]
            y = X + (1.0 if gamma_one else i["gamma"]) * y * branch
        return y

    def model(i):
        pre = i["A"].float() @ i["W"].float().t()
        if epi == "splitk":
            return pre.double()
        y = _act32(pre + i["bias"], act, dtype)
        if epi == "resid":
            y = i["X"] + i["gamma"] * y
        return y.double() if dtype == F32 else round_to(y.double(), dtype)

    def zero_k(k):
        def f(i):
            W = i["W"].clone()
            W[:, k] = 0
            return ref(_with(i, W=W))
        return f

    ks = k_indices(K)
    if epi == "splitk" and k_per_split < K:              # one split of the whole K has no split edge
        ks["k_split_edge"] = k_per_split
    defects = {name: zero_k(k) for name, k in ks.items()}
    for vec in ("bias", "gamma"):
        if vec in inp:
            for name, v in vec_variants(inp[vec]).items():
                defects[f"{vec}_{name}"] = (lambda i, vec=vec, v=v: ref(_with(i, **{vec: v})))
    if epi == "resid":
        defects["branch_15_16"] = lambda i: ref(i, branch=15 / 16)
        defects["gamma_as_one"] = lambda i: ref(i, gamma_one=True)
        if M > 1:
            defects["resid_from_row_before"] = lambda i: ref(i, resid_shift=True)
    if M > 1:
        defects["last_row_from_row_before"] = lambda i: ref(i, last_from_prev=True)
    if epi == "bias_act" and act != 0:
        defects["act_omitted_on_one_column"] = lambda i: ref(i, noact_col=int(inp["bias"].argmin()))
    if epi == "bias_act" and act == 3:
        defects["relu_for_leaky"] = lambda i: ref(i, relu_for_leaky=True)
    family = {"bias_act": "gemm_bias_gelu" if act == 2 else "gemm_bias_act", "resid": "gemm_resid", "splitk": "splitk"}[epi]
    return Case(family, dtype, inp, ref, model, defects, 2.0, flat=SPLITK_BOUND[dtype] if epi == "splitk" else None,
                what=f"gemm {epi} {M}x{N}x{K} act={act}")


# ----------------------------------------------------------------------------- conv as GEMM
def _conv_inputs(n, H, cin, cout, dtype):
    return {"x": q(rnd((n, cin, H, H), 1), dtype),                                     # NCHW here; the test uploads NHWC
            "w": q(rnd((cout, cin, 3, 3), 2, 1 / math.sqrt(9 * cin)), dtype),
            "b": signed((cout,), 3, 0.05, 0.2)}


def _conv3_defects(ref, inp, cin, cout):
    def zero_w(ci, ky, kx):
        def f(i):
            w = i["w"].clone()
            w[:, ci, ky, kx] = 0
            return ref(_with(i, w=w))
        return f
    e = 32                                                  # K index (ky, kx, ci) next to the first K-tile edge
    defects = {"k_first": zero_w(0, 0, 0), "tap22_of_last_cin": zero_w(cin - 1, 2, 2),
               "k_tile_edge": zero_w(e % cin, (e // cin) // 3, (e // cin) % 3)}
    for name, v in vec_variants(inp["b"]).items():
        defects[f"bias_{name}"] = (lambda i, v=v: ref(_with(i, b=v)))
    defects["act_omitted_on_one_column"] = lambda i: ref(i, noact_col=int(inp["b"].argmin()))
    defects["last_row_from_row_before"] = lambda i: ref(i, last_from_prev=True)
    return defects


def _last_from_prev(y):
    """(n, h, w, c): the last pixel takes the result of the pixel before it"""
    y = y.clone()
    flat = y.view(-1, y.shape[-1])
    flat[-1] = flat[-2]
    return y


def conv3x3_s2(n, H, cin, cout, dtype):
    """conv3x3 stride 2 pad 1 + bias + LeakyReLU(0.01) (A_IM2COL3_S2, EPI_BIAS_ACT); NHWC out"""
    inp = _conv_inputs(n, H, cin, cout, dtype)

    def ref(i, noact_col=None, relu_for_leaky=False, last_from_prev=False):
        i = _d(i)
        y = F.conv2d(i["x"], i["w"], i["b"], stride=2, padding=1).permute(0, 2, 3, 1)
        y = _act64(y, 3, noact_col, relu_for_leaky).contiguous()
        return _last_from_prev(y) if last_from_prev else y

    def model(i):
        y = F.conv2d(i["x"], i["w"], i["b"], stride=2, padding=1).permute(0, 2, 3, 1)
        y = torch.where(y >= 0, y, 0.01 * y).double()
        return y if dtype == F32 else round_to(y, dtype)

    defects = _conv3_defects(ref, inp, cin, cout)
    defects["relu_for_leaky"] = lambda i: ref(i, relu_for_leaky=True)
    return Case("conv_s2", dtype, inp, ref, model, defects, 2.0, what=f"conv3 s2 n={n} H={H} {cin}->{cout}")


def conv3x3_pool(n, H, cin, cout, dtype):
    """conv3x3 stride 1 pad 1 + bias + ReLU + maxpool 2 (A_IM2COL3_POOL, EPI_POOL4); NHWC out"""
    inp = _conv_inputs(n, H, cin, cout, dtype)

    def ref(i, noact_col=None, last_from_prev=False, three_of_four=False):
        i = _d(i)
        y = F.conv2d(i["x"], i["w"], i["b"], padding=1).permute(0, 2, 3, 1)
        y = _act64(y, 1, noact_col)
        win = y.reshape(n, H // 2, 2, H // 2, 2, cout).permute(0, 1, 3, 5, 2, 4).reshape(n, H // 2, H // 2, cout, 4)
        y = (win[..., :3] if three_of_four else win).max(-1).values.contiguous()
        return _last_from_prev(y) if last_from_prev else y

    def model(i):
        y = F.max_pool2d(F.relu(F.conv2d(i["x"], i["w"], i["b"], padding=1)), 2).permute(0, 2, 3, 1).double()
        return y if dtype == F32 else round_to(y, dtype)

    defects = _conv3_defects(ref, inp, cin, cout)
    defects["pool_over_three_of_four"] = lambda i: ref(i, three_of_four=True)
    return Case("pool4", dtype, inp, ref, model, defects, 2.0, what=f"conv3 pool n={n} H={H} {cin}->{cout}")


def conv_transpose2x2(n, H, cin, cout, act, dtype):
    """ConvTranspose2d(k = 2, s = 2) + bias + activation (EPI_CONVT); NHWC out"""
    inp = {"x": q(rnd((n, cin, H, H), 1), dtype), "w": q(rnd((cin, cout, 2, 2), 2, 1 / math.sqrt(cin)), dtype),
           "b": signed((cout,), 3, 0.05, 0.2)}

    def ref(i, noact_col=None, relu_for_leaky=False):
        i = _d(i)
        y = F.conv_transpose2d(i["x"], i["w"], i["b"], stride=2).permute(0, 2, 3, 1)
        return _act64(y, act, noact_col, relu_for_leaky).contiguous()

    def model(i):
        y = _act32(F.conv_transpose2d(i["x"], i["w"], i["b"], stride=2).permute(0, 2, 3, 1), act, dtype).double()
        return y if dtype == F32 else round_to(y, dtype)

    def zero_k(k):
        def f(i):
            w = i["w"].clone()
            w[k] = 0
            return ref(_with(i, w=w))
        return f

    def last_from_prev(i):
        x = i["x"].clone()                                  # the last input pixel's row of A is the one before it
        x[n - 1, :, H - 1, H - 1] = x[n - 1, :, H - 1, H - 2]
        return ref(_with(i, x=x))

    defects = {name: zero_k(k) for name, k in k_indices(cin).items()}
    for name, v in vec_variants(inp["b"]).items():
        defects[f"bias_{name}"] = (lambda i, v=v: ref(_with(i, b=v)))
    defects["act_omitted_on_one_column"] = lambda i: ref(i, noact_col=int(inp["b"].argmin()))
    if act == 3:
        defects["relu_for_leaky"] = lambda i: ref(i, relu_for_leaky=True)
    defects["quadrants_dy_dx_swapped"] = lambda i: ref(_with(i, w=i["w"].transpose(2, 3)))
    defects["last_row_from_row_before"] = last_from_prev
    return Case("convt", dtype, inp, ref, model, defects, 2.0, what=f"convT n={n} H={H} {cin}->{cout} act={act}")


# ----------------------------------------------------------------------------- depthwise 7x7 + LayerNorm
DW_KINDS = ("tile", "tiny", "tiny_pair", "roll", "mfma", "pair")      # gcv_dw_plan's kind codes (include/genconvit_hip.h)


def dw_plan(dtype, n, H, W, C, aligned=True):
    """(kind, rows per band) of the kernel gcv_k_dwconv7_ln runs for this launch, asked of the library's own planner (host
    code, no GPU); rows per band is 0 for the kinds without bands"""
    import ctypes
    from genconvit_amd import _lib
    out = (ctypes.c_int * 5)()
    _lib.check(_lib.load().gcv_dw_plan(_lib.dtype_code(dtype), n, H, W, C, int(aligned), out), "gcv_dw_plan")
    return DW_KINDS[out[0]], out[4]


def dwconv7_ln(C, H, W, n, dtype, aligned=True, plan_nimg=0):
    """depthwise 7x7 pad 3 + bias + LayerNorm(C, eps 1e-6); x NCHW here (the test uploads NHWC), NHWC out.  The taps are
    uploaded in fp32.  The matrix-pipe kernel (csrc/dwconv_mfma.h, 16-bit storage) rounds them to the storage dtype, being
    an MFMA operand; for a launch that gcv_dw_plan sends there, reference, model and defects round them too.  plan_nimg > 0:
    the launch is gcv_k_dwconv7_ln_planned's, n images under the plan (kernel, rows per band) of plan_nimg images.  With
    more than one band per image the two band-seam defects join the catalogue, built from the plan's rows per band:
    case.kind and case.band_rows say what was planned."""
    inp = {"x": q(rnd((n, C, H, W), 1, 2.0), dtype), "w": signed((C, 1, 7, 7), 2, 0.05, 0.25),
           "b": signed((C,), 3, 0.1, 0.3), "lw": rnd((C,), 4, 0.5) + 1.0, "lb": signed((C,), 5, 0.1, 0.3)}
    kind, band_rows = dw_plan(dtype, plan_nimg if plan_nimg > 0 else n, H, W, C, aligned)
    taps_in_T = kind == "mfma"

    cache = {}

    def conv(i, clamp_right=False):
        """the depthwise conv + bias in float64, NHWC; the clean inputs' result is kept (the matrix-pipe cases are large)"""
        keep = not clamp_right and all(i[k] is inp[k] for k in ("x", "w", "b"))
        if keep and "y" in cache:
            return cache["y"]
        d = _d({k: (q(i[k], dtype) if (k == "w" and taps_in_T) else i[k]) for k in ("x", "w", "b")})
        if clamp_right:
            xp = F.pad(d["x"], (3, 3, 3, 3))
            xp[:, :, 3:H + 3, W + 3:] = d["x"][:, :, :, W - 1:]      # the last column again where zeros belong
            y = F.conv2d(xp, d["w"], d["b"], groups=C)
        else:
            y = F.conv2d(d["x"], d["w"], d["b"], padding=3, groups=C)
        y = y.permute(0, 2, 3, 1).contiguous()
        if keep:
            cache["y"] = y
        return y

    def ref(i, clamp_right=False, last_from_prev=False, y=None):
        y = conv(i, clamp_right) if y is None else y
        if last_from_prev:
            y = _last_from_prev(y)
        return numutil.ln_ref(y, i["lw"].double(), i["lb"].double(), 1e-6).contiguous()

    # band seams: band 1 of the last image, output rows r0 ... r1 - 1
    r0, r1 = band_rows, min(2 * band_rows, H)

    def band_head_without_rows_above(i):
        """the first output rows of band 1 (those whose taps reach above it) computed as if the map began at the band"""
        d = _d({k: (q(i[k], dtype) if (k == "w" and taps_in_T) else i[k]) for k in ("x", "w", "b")})
        top = min(r0 + 3, r1)                               # output rows r0 ... top - 1 read input rows above r0
        rows = F.conv2d(F.pad(d["x"][n - 1:, :, r0:top + 3], (3, 3, 3, max(0, top + 3 - H))), d["w"], d["b"], groups=C)
        y = conv(i).clone()
        y[n - 1, r0:top] = rows.permute(0, 2, 3, 1)[0, :top - r0]
        return ref(i, y=y)

    def band_last_row_from_row_before(i):
        y = conv(i).clone()
        y[n - 1, r1 - 1] = y[n - 1, r1 - 2]
        return ref(i, y=y)

    def model(i):
        y = F.conv2d(i["x"], q(i["w"], dtype) if taps_in_T else i["w"], i["b"], padding=3, groups=C).permute(0, 2, 3, 1)
        y = F.layer_norm(y, (C,), i["lw"], i["lb"], 1e-6).double()
        return y if dtype == F32 else round_to(y, dtype)

    def tap_zeroed(i):
        y = conv(i).clone()                                 # the centre tap of the last channel: on data at every map size
        wc = (q(i["w"], dtype) if taps_in_T else i["w"]).double()[C - 1, 0, 3, 3]
        y[..., C - 1] -= wc * i["x"].double()[:, C - 1]
        return ref(i, y=y)

    def bias_zeroed(i):
        y = conv(i).clone()
        y[..., C - 1] -= i["b"].double()[C - 1]
        return ref(i, y=y)

    defects = {"one_tap_zeroed_on_one_channel": tap_zeroed, "dw_bias_zeroed_on_one_channel": bias_zeroed}
    if W > 1:
        defects["right_edge_clamped"] = lambda i: ref(i, clamp_right=True)
    for vec in ("lw", "lb"):
        for name, v in vec_variants(inp[vec]).items():
            defects[f"{vec}_{name}"] = (lambda i, vec=vec, v=v: ref(_with(i, **{vec: v})))
    if n * H * W > 1:
        defects["last_row_from_row_before"] = lambda i: ref(i, last_from_prev=True)
    if 0 < band_rows < H:                                   # a band kernel with a seam inside the image
        defects["band_head_without_rows_above"] = band_head_without_rows_above
        defects["band_last_row_from_row_before"] = band_last_row_from_row_before
    case = Case("dw_ln", dtype, inp, ref, model, defects, 3.0,
                what=f"dwconv_ln C={C} {H}x{W} n={n}" + (f" planned as {plan_nimg} images" if plan_nimg > 0 else ""))
    case.kind, case.band_rows = kind, band_rows
    return case


# ----------------------------------------------------------------------------- fused ConvNeXt MLP
MLP_KINDS = ("gemm", "fused96", "xs192", "pair384")      # gcv_mlp_plan's kind codes (include/genconvit_hip.h)


def mlp_plan(dtype, C, M, wg_cap=256):
    """gcv_mlp_plan: (kind, seven fields by kind) of the ConvNeXt MLP at M tokens, the persistent kernels held to wg_cap
    workgroups (256: the networks' launch); host code, no GPU"""
    import ctypes
    from genconvit_amd import _lib
    out = (ctypes.c_int * 8)()
    _lib.check(_lib.load().gcv_mlp_plan(_lib.dtype_code(dtype), C, M, wg_cap, out), "gcv_mlp_plan")
    return (MLP_KINDS[out[0]],) + tuple(out[1:])


def xs_pw1_range(C, M):
    """width of the hidden ranges the C = 384 pw1 kernel's workgroups own at M tokens: 32-wide chunks per workgroup as
    gcv_mlp_plan reports them (csrc/mlp_pair.h, xs_pw1_pick_split)"""
    plan = mlp_plan(F16, C, M)
    assert plan[0] == "pair384", plan
    return 32 * plan[3]


# ---- launch geometry of the MLP kernels (tests/census.py; tests/test_host_cpu.py asserts that the networks reach exactly
# the geometries these lists cover).  C = 384, keyed (hidden-range split ns, pw2 tile (BN, D, TB)): the token counts of
# test_fused_mlp_layerscale_residual (PAIR384_M); for the splits ns = 12, 6, 4, 2 which those leave out, the smallest token
# count with that split (PAIR384_SPLIT_M); and for the splits that the networks also run beside another pw2 tile, the
# smallest token count with that pair (PAIR384_TILE_M).  Each is one token more than a whole number of 256-token tiles.
PAIR384_M = [128, 1000, 6272, 40000, 60013]      # ns 24, 24, 8, 3, 1; pw2 tiles (192, 5, 4) x 3, (192, 4, 8), (384, 3, 8)
PAIR384_SPLIT_M = [2561, 8193, 10753, 21761]     # ns 12, 6, 4, 2: 4, 8, 12 and 24 chunks per workgroup on the ring of six
PAIR384_TILE_M = [16129, 45825, 81921, 87297]    # ns 4 + (192, 4, 8); ns 4, 3, 2 + the full-width (384, 3, 8)
# The persistent kernels, (C, segments or token count, workgroup cap): xs_mlp_kernel (C = 192) and fused_mlp_res_kernel (C = 96,
# from 65 536 tokens) plain and with the LN-patchify epilogue at one, two and three or more passes per workgroup / tiles per
# wave.  gcv_k_fused_mlp*_planned holds the launch to `cap` workgroups, so that 2 352 and 69 000 tokens run the four and
# five passes that a batch of 128 runs on 256.
PERSISTENT = [
    (192, 2352, 256), (192, 2352, 5), (192, 2352, 3),                                        # 10 passes: 1, 2, 4 per workgroup
    (192, [(3, 28, 28)], 256), (192, [(3, 28, 28)], 5), (192, [(5, 28, 28), (5, 14, 14)], 6),   # 10, 10, 20 passes: 1, 2, 4
    (96, 65536, 256), (96, 70013, 256), (96, 70013, 64),                                     # 2 048 / 2 188 wave tiles: 1, 2, 5
    (96, [(64, 32, 32)], 256), (96, [(22, 56, 56)], 256), (96, [(21, 56, 56), (9, 28, 28), (3, 14, 14)], 64),   # 1, 2, 5
]


def persistent_key(dtype, C, shape, wg_cap):
    """(kernel, epilogue, passes per workgroup or tiles per wave as 1 / 2 / 3-and-more) of a PERSISTENT entry"""
    segs = shape if isinstance(shape, list) else None
    M = sum(n * h * w for n, h, w in segs) if segs else shape
    plan = mlp_plan(dtype, C, M, wg_cap)
    if plan[0] == "xs192":
        return ("xs192", "lnp" if segs else "plain", min(plan[3], 3))
    assert plan[0] == "fused96" and plan[1] == 1, (C, M, plan)
    return ("res96", "lnp" if segs else "plain", min(plan[4], 3))


def lnp_index(segs):
    """token index of each (patch row, quadrant) behind the LN-patchify epilogue: (M / 4, 4), quadrant = 2 dy + dx"""
    rows, t = [], 0
    for n, H, W in segs:
        img, py, px = torch.meshgrid(torch.arange(n), torch.arange(H // 2), torch.arange(W // 2), indexing="ij")
        base = t + img * (H * W) + 2 * py * W + 2 * px
        rows.append(torch.stack([base, base + 1, base + W, base + W + 1], -1).reshape(-1, 4))
        t += n * H * W
    return torch.cat(rows)


def fused_mlp(C, M, dtype, segs=None, b2_range=(0.25, 0.5)):
    """fc1 -> exact GELU -> (rounded to T) -> fc2 -> * gamma -> + shortcut (gcv_k_fused_mlp); at C = 384 the kernel pair's fc2
    weight is T(gamma * W2), and the reference rounds that product as the packer does.  With `segs` ((images, H, W)
    per segment, M their token count) the stage boundary's LayerNorm2d(eps 1e-6) and 2x2 space-to-depth follow
    (gcv_k_fused_mlp_lnp): (M / 4, 4 C) out.  The reference keeps pre-activation, hidden and fc2 product of the clean inputs
    and derives each defect from them by the rank-one (or 32-wide) update that the defect is, so that the 70 000-token cases
    stay affordable; a defect in front of the GELU repeats the GELU and fc2."""
    assert dtype in (F16, BF16)
    inp = {"x": q(rnd((M, C), 1, 1.5), dtype),
           "w1": q(rnd((4 * C, C), 2, 1 / math.sqrt(C)), dtype),
           "w2": q(rnd((C, 4 * C), 3, 1 / math.sqrt(4 * C)), dtype),
           "b1": signed((4 * C,), 4, 0.75, 1.5), "b2": signed((C,), 5, *b2_range), "gamma": signed((C,), 6, 0.25, 0.5),
           "res": q(rnd((M, C), 7, 0.25), dtype)}
    if segs is not None:
        assert M == sum(n * h * w for n, h, w in segs)
        inp["lw"], inp["lb"] = rnd((C,), 8, 0.5) + 1.0, signed((C,), 9, 0.1, 0.3)
        index = lnp_index(segs)
    cache = {}
    fold = C == 384      # the kernel pair multiplies by T(gamma * W2), rounded once when the weights are packed (mlp_pair.h)

    def hidden(pre):
        return numutil.gelu_ref(pre).to(dtype).double()

    def w2g(i, gamma_one=False):
        """what GEMM2 multiplies the hidden by, layer scale included; (C, 4C) float64"""
        if gamma_one:
            return i["w2"].double()
        if fold:
            return q(i["gamma"][:, None] * i["w2"], dtype).double()
        return i["gamma"].double()[:, None] * i["w2"].double()

    def stages(i):
        """pre-activation, hidden, and gamma (W2 . h) of the case's own inputs"""
        if "pre" not in cache:
            d = _d(i)
            cache["pre"] = d["x"] @ d["w1"].t() + d["b1"]
            cache["h"] = hidden(cache["pre"])
            cache["zg"] = cache["h"] @ w2g(i).t()
        return cache["pre"], cache["h"], cache["zg"]

    def tail(i, zg, branch=1.0, gamma_one=False, last_from_prev=False, resid_shift=False, idx=None):
        d = _d({k: v for k, v in i.items() if k in ("b2", "gamma", "res", "lw", "lb")})
        br = zg + (1.0 if gamma_one else d["gamma"]) * d["b2"]
        res = d["res"]
        if last_from_prev:
            br = br.clone()
            br[M - 1] = br[M - 2]
        if resid_shift:
            res = res.clone()
            res[M - 1] = res[M - 2]
        y = res + br * branch
        if segs is None:
            return y
        yn = numutil.ln_ref(y, d["lw"], d["lb"], 1e-6)      # the residual stream stays fp32 in registers: no rounding of y
        return yn[index if idx is None else idx].reshape(-1, 4 * C)

    def ref(i, **kw):
        if i is inp:
            return tail(i, stages(i)[2], **kw)
        d = _d(i)                                           # other inputs than the case's own: from scratch
        return tail(i, hidden(d["x"] @ d["w1"].t() + d["b1"]) @ w2g(i).t(), **kw)

    def model(i):
        pre = i["x"] @ i["w1"].t() + i["b1"]
        packed = not (C == 96 and M < 65536)                # fused_mlp_kernel<T, 96, 4> ends in the fp32 finish (numutil)
        h = numutil.gelu_h16_ref(pre, dtype, packed_finish=packed).float()
        if fold:
            y = i["res"] + (h @ q(i["gamma"][:, None] * i["w2"], dtype).t() + i["gamma"] * i["b2"])
        else:
            y = i["res"] + i["gamma"] * (h @ i["w2"].t() + i["b2"])
        if segs is not None:
            y = F.layer_norm(y, (C,), i["lw"], i["lb"], 1e-6)[index].reshape(-1, 4 * C)
        return round_to(y.double(), dtype)

    def fc1_k(k):
        def f(i):
            pre, _, _ = stages(i)
            d = _d(i)
            return tail(i, hidden(pre - torch.outer(d["x"][:, k], d["w1"][:, k])) @ w2g(i).t())
        return f

    def b1_as(v):
        def f(i):
            pre, _, _ = stages(i)
            return tail(i, hidden(pre + (v.double() - i["b1"].double())) @ w2g(i).t())
        return f

    def hidden_dropped(j0, j1):
        def f(i):
            _, h, zg = stages(i)
            return tail(i, zg - h[:, j0:j1] @ w2g(i)[:, j0:j1].t())
        return f

    def gamma_as(v):
        def f(i):
            i2 = _with(i, gamma=v)
            return tail(i2, stages(i)[1] @ w2g(i2).t())
        return f

    width = xs_pw1_range(C, M) if C == 384 else 32
    defects = {f"fc1_{name}": fc1_k(k) for name, k in k_indices(C).items()}
    defects["one_hidden_unit_dropped"] = hidden_dropped(4 * C - 31, 4 * C - 30)
    defects[f"last_{width}_hidden_units_dropped"] = hidden_dropped(4 * C - width, 4 * C)
    for name, v in vec_variants(inp["b1"]).items():
        defects[f"b1_{name}"] = b1_as(v)
    for name, v in vec_variants(inp["gamma"]).items():
        defects[f"gamma_{name}"] = gamma_as(v)
    for vec in ("b2",) + (("lw", "lb") if segs is not None else ()):
        for name, v in vec_variants(inp[vec]).items():
            defects[f"{vec}_{name}"] = (lambda i, vec=vec, v=v: tail(_with(i, **{vec: v}), stages(i)[2]))
    defects["branch_15_16"] = lambda i: tail(i, stages(i)[2], branch=15 / 16)
    defects["gamma_as_one"] = lambda i: tail(i, stages(i)[1] @ w2g(i, gamma_one=True).t(), gamma_one=True)
    if M > 1:
        defects["last_row_from_row_before"] = lambda i: tail(i, stages(i)[2], last_from_prev=True)
        defects["resid_from_row_before"] = lambda i: tail(i, stages(i)[2], resid_shift=True)
    if segs is not None:
        defects["quadrants_dy_dx_swapped"] = lambda i: tail(i, stages(i)[2], idx=index[:, [0, 2, 1, 3]])
        if len(segs) > 1 and segs[1][2] != segs[0][2]:
            def prev_geometry(i):
                idx = index.clone()
                r = sum(n * (h // 2) * (w // 2) for n, h, w in segs[:1])     # first patch row of the second segment ...
                t0, wprev = segs[0][0] * segs[0][1] * segs[0][2], segs[0][2]
                idx[r] = torch.tensor([t0, t0 + 1, t0 + wprev, t0 + wprev + 1])   # ... with the first segment's width
                return tail(i, stages(i)[2], idx=idx)
            defects["segment_start_with_previous_geometry"] = prev_geometry
    family, scale = ("mlp", 2.0) if segs is None else ("mlp_lnp", 4.0)
    return Case(family, dtype, inp, ref, model, defects, scale,
                what=f"fused mlp C={C} M={M}" + (f" + LN-patchify {segs}" if segs is not None else ""))


# ----------------------------------------------------------------------------- the small kernels of the verdict path
class MultiCase:
    """A family with several outputs (reparam: mu, z; resize + MSE: recon, msepart, mse).  ref, model and every defect return
    name -> float64 tensor; `parts` holds one Case per output, which is that output's comparator.  A defect counts as
    rejected when any output rejects it."""

    def __init__(self, what, dtype, inputs, ref, model, defects, parts):
        self.what, self.dtype, self.inputs, self.ref, self.model, self.defects = f"{what} {NAMES[dtype]}", dtype, inputs, ref, model, defects
        self.parts = parts
        self._want = None

    def want(self):
        if self._want is None:
            self._want = self.ref(self.inputs)
        return self._want

    def assert_close(self, got):
        """got: name -> device tensor; an output the launch did not write is left out"""
        for name, g in got.items():
            ok, msg = self.parts[name].check(g, self.want()[name], self.inputs)
            print(msg)
            assert ok, msg


def _vec_defects(defects, inp, ref, names):
    for vec in names:
        for name, v in vec_variants(inp[vec]).items():
            defects[f"{vec}_{name}"] = (lambda i, vec=vec, v=v: ref(_with(i, **{vec: v})))


def _out(y, dtype):
    """a float32 model result as the output buffer holds it; float64"""
    return y.double() if dtype == F32 else round_to(y.double(), dtype)


def stem(C, n, Ho, Wo, layout, dtype):
    """conv 4x4 stride 4 (3 -> C) + bias + LayerNorm(C, eps 1e-6): gcv_k_stem_ln_c.  x NCHW here; `layout` is how the test
    uploads it and changes no value.  (n Ho Wo, C) out, token-major.  The weights are rounded to the storage dtype: 16-bit
    storage runs the stem on the matrix pipe, where they are an MFMA operand.  The conv is the contraction of each token's
    48 patch values (k = ci 16 + ky 4 + kx) with w.  x is +-[0.5, 2]: a single token has to show a zeroed w[:, k]."""
    T = n * Ho * Wo
    inp = {"x": q(signed((n, 3, 4 * Ho, 4 * Wo), 1, 0.5, 2.0), dtype), "w": q(rnd((C, 3, 4, 4), 2, 0.2), dtype),
           "bias": signed((C,), 3, 0.1, 0.3), "lw": rnd((C,), 4, 0.5) + 1.0, "lb": signed((C,), 5, 0.1, 0.3)}

    def patches(x):
        return x.reshape(n, 3, Ho, 4, Wo, 4).permute(0, 2, 4, 1, 3, 5).reshape(T, 48)

    def ref(i, last_from_prev=False):
        d = _d(i)
        y = patches(d["x"]) @ d["w"].reshape(C, 48).t() + d["bias"]
        if last_from_prev:
            y = y.clone()
            y[-1] = y[-2]
        return numutil.ln_ref(y, d["lw"], d["lb"], 1e-6)

    def model(i):
        y = F.conv2d(i["x"], i["w"], i["bias"], stride=4).permute(0, 2, 3, 1).reshape(T, C)
        return _out(F.layer_norm(y, (C,), i["lw"], i["lb"], 1e-6), dtype)

    def zero_k(k):
        def f(i):
            w = i["w"].reshape(C, 48).clone()
            w[:, k] = 0
            return ref(_with(i, w=w.reshape(C, 3, 4, 4)))
        return f

    defects = {"k_first": zero_k(0), "k_last": zero_k(47), "k_channel_and_step_edge": zero_k(16),
               "kx_ky_transposed": lambda i: ref(_with(i, w=i["w"].transpose(2, 3)))}
    _vec_defects(defects, inp, ref, ("bias", "lw", "lb"))
    if T > 1:
        defects["last_row_from_row_before"] = lambda i: ref(i, last_from_prev=True)
    return Case("stem", dtype, inp, ref, model, defects, 3.0, what=f"stem C={C} n={n} {Ho}x{Wo} {layout}")


def ln_patchify(C, H, W, n, dtype):
    """LayerNorm2d(C, eps 1e-6) + 2x2 space-to-depth, an odd last row / column dropped (gcv_k_ln_patchify): x (n, H, W, C) ->
    (n, H / 2, W / 2, 4 C), K index (2 dy + dx) C + c"""
    Ho, Wo = H // 2, W // 2
    inp = {"x": q(rnd((n, H, W, C), 1, 2.0), dtype), "lw": rnd((C,), 4, 0.5) + 1.0, "lb": signed((C,), 5, 0.1, 0.3)}

    def gather(y, swap=False, keep_last_col=False, last_from_prev=False):
        o = y[:, :2 * Ho, :2 * Wo].reshape(n, Ho, 2, Wo, 2, C)
        o = (o.permute(0, 1, 3, 4, 2, 5) if swap else o.permute(0, 1, 3, 2, 4, 5)).reshape(n * Ho * Wo * 4, C).clone()
        if keep_last_col:                 # pixel (iy, W - 1) written as well, at the index the gather gives it: patch column Wo
            for b in range(n):
                for iy in range(2 * Ho):
                    at = ((b * Ho + iy // 2) * Wo + (W - 1) // 2) * 4 + (iy & 1) * 2 + ((W - 1) & 1)
                    if at < o.shape[0]:
                        o[at] = y[b, iy, W - 1]
        o = o.reshape(n * Ho * Wo, 4 * C)
        if last_from_prev:
            o[-1] = o[-2]
        return o.reshape(n, Ho, Wo, 4 * C)

    def ref(i, **kw):
        return gather(numutil.ln_ref(i["x"], i["lw"], i["lb"], 1e-6), **kw)

    def model(i):
        return _out(gather(F.layer_norm(i["x"], (C,), i["lw"], i["lb"], 1e-6)), dtype)

    defects = {}
    _vec_defects(defects, inp, ref, ("lw", "lb"))
    defects["quadrants_dy_dx_swapped"] = lambda i: ref(i, swap=True)
    if W % 2 and n * Ho > 1:            # with a single patch row every such write lands behind the output: the test's sentinel
        defects["dropped_last_column_kept"] = lambda i: ref(i, keep_last_col=True)
    if n * Ho * Wo > 1:
        defects["last_row_from_row_before"] = lambda i: ref(i, last_from_prev=True)
    return Case("ln_patchify", dtype, inp, ref, model, defects, 3.0, what=f"ln_patchify C={C} {H}x{W} n={n}")


POOL_SENTINEL = 7.0


def pool_ln(C, HW, nimg, dtype, seg_n=0, row_stride=1, row0=0):
    """mean over the HW tokens + LayerNorm(C, eps 1e-6): gcv_k_pool_ln, and with seg_n > 0 gcv_k_pool_ln_rows, which writes image b
    to row case.rows[b] = (b % seg_n) row_stride + row0 + b / seg_n.  (nimg, C) out in image order: the test gathers
    out[case.rows].  LayerNorm takes a scaled row to the same result but for eps, so a mean divided by HW + 1 shows only
    where the variance over the channels is of eps' size: image 0 is scaled to a pooled variance of about eps / 2."""
    x = rnd((nimg, HW, C), 1, 2.0)
    x[0] *= 6e-4 * math.sqrt(HW)           # pooled values of std 2 / sqrt(3 HW) x that = 6.9e-4: variance 0.48e-6
    inp = {"x": q(x, dtype), "lw": rnd((C,), 4, 0.5) + 1.0, "lb": signed((C,), 5, 0.1, 0.3)}
    rows = [b if seg_n <= 0 else (b % seg_n) * row_stride + row0 + b // seg_n for b in range(nimg)]

    def ref(i, drop_last=False, div_plus_1=False, last_from_prev=False, plain_rows=False):
        d = _d(i)
        xs = d["x"][:, :HW - 1] if drop_last else d["x"]
        m = xs.sum(1) / ((HW + 1) if div_plus_1 else xs.shape[1])
        if last_from_prev:
            m = m.clone()
            m[-1] = m[-2]
        y = numutil.ln_ref(m, d["lw"], d["lb"], 1e-6)
        if plain_rows:                    # image b written to row b: row rows[b] holds image rows[b], or was never written
            y = torch.stack([y[r] if r < nimg else torch.full_like(y[0], POOL_SENTINEL) for r in rows])
        return y

    def model(i):
        return _out(F.layer_norm(i["x"].mean(1), (C,), i["lw"], i["lb"], 1e-6), dtype)

    defects = {}
    _vec_defects(defects, inp, ref, ("lw", "lb"))
    if HW > 1:
        defects["last_token_left_out_of_the_mean"] = lambda i: ref(i, drop_last=True)
    defects["mean_divided_by_HW_plus_1"] = lambda i: ref(i, div_plus_1=True)
    if nimg > 1:
        defects["last_row_from_row_before"] = lambda i: ref(i, last_from_prev=True)
    if seg_n > 0:
        defects["rows_in_plain_order"] = lambda i: ref(i, plain_rows=True)
    case = Case("pool_ln", dtype, inp, ref, model, defects, 3.0,
                what=f"pool_ln C={C} HW={HW} n={nimg}" + (f" rows {rows}" if seg_n > 0 else ""))
    case.rows = rows
    return case


def conv3_first(n, H, W, pool, dtype, strides="nchw"):
    """Conv2d(3, 16, 3, pad 1) as the autoencoders' first layer (gcv_k_conv3_first): pool: stride 1 + ReLU + maxpool 2;
    else stride 2 + LeakyReLU(0.01).  x NCHW here, `strides` is how the test addresses it; (n, H / 2, W / 2, 16) out.  The
    weights are rounded to the storage dtype (an MFMA operand in 16-bit storage).  At even H, W the stride-2 conv reads the
    padding on the left and on top only: its clamped-edge defects are those two."""
    inp = {"x": q(rnd((n, 3, H, W), 1, 2.0), dtype), "w": q(rnd((16, 3, 3, 3), 2, 0.3), dtype),
           "bias": signed((16,), 3, 0.1, 0.3)}
    act = 1 if pool else 3

    def ref(i, noact_col=None, relu_for_leaky=False, three_of_four=False, clamp=None, last_from_prev=False):
        d = _d(i)
        xp = F.pad(d["x"], (1, 1, 1, 1))
        if clamp == "right":
            xp[:, :, 1:H + 1, W + 1] = d["x"][:, :, :, W - 1]
        elif clamp == "bottom":
            xp[:, :, H + 1, 1:W + 1] = d["x"][:, :, H - 1, :]
        elif clamp == "left":
            xp[:, :, 1:H + 1, 0] = d["x"][:, :, :, 0]
        elif clamp == "top":
            xp[:, :, 0, 1:W + 1] = d["x"][:, :, 0, :]
        y = F.conv2d(xp, d["w"], d["bias"], stride=1 if pool else 2).permute(0, 2, 3, 1)
        y = _act64(y, act, noact_col, relu_for_leaky)
        if pool:
            win = y.reshape(n, H // 2, 2, W // 2, 2, 16).permute(0, 1, 3, 5, 2, 4).reshape(n, H // 2, W // 2, 16, 4)
            y = (win[..., :3] if three_of_four else win).max(-1).values
        y = y.contiguous()
        return _last_from_prev(y) if last_from_prev else y

    def model(i):
        if pool:
            y = F.max_pool2d(F.relu(F.conv2d(i["x"], i["w"], i["bias"], padding=1)), 2)
        else:
            y = F.leaky_relu(F.conv2d(i["x"], i["w"], i["bias"], stride=2, padding=1), 0.01)
        return _out(y.permute(0, 2, 3, 1), dtype)

    def zero_w(ci, ky, kx):
        def f(i):
            w = i["w"].clone()
            w[:, ci, ky, kx] = 0
            return ref(_with(i, w=w))
        return f

    # rows of wp are k = (ky 3 + kx) 3 + ci; the matrix-pipe kernel's k is ci 9 + ky 3 + kx, a lane group per 8 of them
    defects = {"wp_row_0": zero_w(0, 0, 0), "wp_row_26": zero_w(2, 2, 2), "mfma_k_8": zero_w(0, 2, 2),
               "mfma_k_16": zero_w(1, 2, 1), "mfma_k_24": zero_w(2, 2, 0),
               "kx_ky_transposed": lambda i: ref(_with(i, w=i["w"].transpose(2, 3)))}
    _vec_defects(defects, inp, ref, ("bias",))
    defects["act_omitted_on_one_column"] = lambda i: ref(i, noact_col=int(inp["bias"].argmin()))
    if pool:
        defects["pool_over_three_of_four"] = lambda i: ref(i, three_of_four=True)
    else:
        defects["relu_for_leaky"] = lambda i: ref(i, relu_for_leaky=True)
    for side in (("right", "bottom") if pool else ("left", "top")):
        defects[f"{side}_edge_clamped"] = lambda i, side=side: ref(i, clamp=side)
    defects["last_row_from_row_before"] = lambda i: ref(i, last_from_prev=True)
    return Case("conv3_first", dtype, inp, ref, model, defects, 3.0,
                what=f"conv3_first {'pool' if pool else 's2'} n={n} {H}x{W} {strides}")


def convt2_small(n, H, W, act, dtype):
    """ConvTranspose2d(16, 3, k = 2, s = 2) + bias + activation, the decoders' last layer (gcv_k_convt2_small); x NCHW here
    (the test uploads NHWC), (n, 2 H, 2 W, 3) out.  The weights stay fp32 in every storage dtype."""
    inp = {"x": q(rnd((n, 16, H, W), 1, 2.0), dtype), "w": rnd((16, 3, 2, 2), 2, 0.3), "bias": signed((3,), 3, 0.1, 0.3)}

    def ref(i, noact_col=None, relu_for_leaky=False):
        d = _d(i)
        y = F.conv_transpose2d(d["x"], d["w"], d["bias"], stride=2).permute(0, 2, 3, 1)
        return _act64(y, act, noact_col, relu_for_leaky).contiguous()

    def model(i):
        return _out(_act32(F.conv_transpose2d(i["x"], i["w"], i["bias"], stride=2).permute(0, 2, 3, 1), act, dtype), dtype)

    def zero_ci(ci):
        def f(i):
            w = i["w"].clone()
            w[ci] = 0
            return ref(_with(i, w=w))
        return f

    def last_from_prev(i):
        px = i["x"].permute(0, 2, 3, 1).reshape(-1, 16).clone()     # pixels in the order the kernel walks them
        px[-1] = px[-2]
        return ref(_with(i, x=px.reshape(n, H, W, 16).permute(0, 3, 1, 2)))

    defects = {f"ci_{ci}": zero_ci(ci) for ci in (0, 15, 4, 8, 12)}      # 4, 8, 12: the packed branch's four-channel passes
    _vec_defects(defects, inp, ref, ("bias",))
    defects["act_omitted_on_one_column"] = lambda i: ref(i, noact_col=int(inp["bias"].argmin()))
    if act == 3:
        defects["relu_for_leaky"] = lambda i: ref(i, relu_for_leaky=True)
    defects["quadrants_dy_dx_swapped"] = lambda i: ref(_with(i, w=i["w"].transpose(2, 3)))
    if n * H * W > 1:
        defects["last_row_from_row_before"] = last_from_prev
    return Case("convt2_small", dtype, inp, ref, model, defects, 3.0, what=f"convt2_small n={n} {H}x{W} act={act}")


REPARAM_N = 12544


def reparam(B, S, dtype):
    """mu = sum of S split-K slabs + bias (fp32 out, flat 1e-5); z = eps exp(0.5 mu) + mu in the storage dtype, written
    hw 256 + c for n = c 49 + hw (gcv_k_reparam).  eps is +-[0.5, 2], so that a wrong exponent shows at every element."""
    N = REPARAM_N
    inp = {"part": rnd((S, B, N), 1, 0.4), "bias": signed((N,), 2, 0.05, 0.2), "eps": signed((B, N), 3, 0.5, 2.0)}

    def nhwc(z, transposed=False):
        z = z.reshape(B, 256, 7, 7)
        if transposed:
            z = z.transpose(2, 3)
        return z.reshape(B, 256, 49).permute(0, 2, 1).reshape(B, N)

    def ref(i, slabs=S, whole_mu=False, eps_shift=False, order="nhwc"):
        d = _d(i)
        mu = d["part"][:slabs].sum(0) + d["bias"]
        eps = d["eps"]
        if eps_shift:
            eps = eps.clone()
            eps[B - 1] = eps[B - 2]
        z = eps * torch.exp(mu if whole_mu else 0.5 * mu) + mu
        return {"mu": mu, "z": z if order == "chw" else nhwc(z, transposed=order == "transposed")}

    def model(i):
        mu = i["part"].sum(0) + i["bias"]
        return {"mu": mu.double(), "z": _out(nhwc(i["eps"] * torch.exp(0.5 * mu) + mu), dtype)}

    defects = {"last_slab_dropped": lambda i: ref(i, slabs=S - 1)}
    _vec_defects(defects, inp, ref, ("bias",))
    defects["exp_of_mu"] = lambda i: ref(i, whole_mu=True)
    if B > 1:
        defects["last_row_eps_from_row_before"] = lambda i: ref(i, eps_shift=True)
    defects["z_left_in_chw_order"] = lambda i: ref(i, order="chw")
    defects["z_with_7x7_transposed"] = lambda i: ref(i, order="transposed")
    what = f"reparam B={B} S={S}"
    parts = {"mu": Case("reparam", dtype, inp, None, None, None, 1.0, flat=1e-5, what=what + " mu"),
             "z": Case("reparam", dtype, inp, None, None, None, 8.0, what=what + " z")}
    return MultiCase(what, dtype, inp, ref, model, defects, parts)


def _head_defects(defects, inp, ref, B, K):
    def zero_k(k):
        def f(i):
            w = i["w"].clone()
            w[:, k] = 0
            return ref(_with(i, w=w))
        return f
    for k in (0, K - 1, 64, 256):          # 64: head_tail_kernel's lane stride; 256: head_tail_splitk_kernel's thread stride
        if k < K:
            defects[f"w_k_{k}"] = zero_k(k)
    defects["w_rows_swapped"] = lambda i: ref(_with(i, w=i["w"].flip(0)))
    defects["biases_swapped"] = lambda i: ref(_with(i, b=i["b"].flip(0)))
    if B > 1:
        defects["last_row_from_row_before"] = lambda i: ref(i, last_from_prev=True)


def head_tail(B, K, dtype):
    """logits = h W^T + b, K -> 2 (gcv_k_head_tail); fp32 out, flat 1e-5 in every storage dtype.  h is +-[0.25, 1]: a single row
    has to show a zeroed w[:, k]."""
    inp = {"h": q(signed((B, K), 1, 0.25, 1.0), dtype), "w": signed((2, K), 2, 0.02, 0.05), "b": signed((2,), 3, 0.1, 0.3)}

    def ref(i, last_from_prev=False):
        d = _d(i)
        y = d["h"] @ d["w"].t() + d["b"]
        if last_from_prev:
            y = y.clone()
            y[B - 1] = y[B - 2]
        return y

    def model(i):
        return (i["h"] @ i["w"].t() + i["b"]).double()

    defects = {}
    _head_defects(defects, inp, ref, B, K)
    return Case("head_tail", dtype, inp, ref, model, defects, 1.0, flat=1e-5, what=f"head_tail B={B} K={K}")


HEAD_SPLITK_BEFORE = {F32: 1e-5, F16: 2e-4, BF16: 2e-3}       # the flat bounds of the test this replaces


def _tie_distance(v, dtype):
    """distance of a float64 value to the nearest midpoint between two neighbouring values of `dtype`"""
    u = numutil.ulp(v, dtype)
    f = v.abs() / u
    return ((f - f.floor()) - 0.5).abs() * u


def head_tail_splitk(B, K, S, act, dtype):
    """h = T(act(sum of S slabs + b1)), logits = h W^T + b (gcv_k_head_tail_splitk); fp32 out.  The reference rounds h to the
    storage dtype as the kernel does.  A hidden unit whose exact value lies next to a rounding tie of T may legitimately
    round the other way and moves a logit by |w| ulp_T(h): the bound of row r is
        1e-5 + sum over the units k of row r within delta of a tie of |w[c, k]| ulp_T(h[k]),
    delta = 4 x the largest |act32(pre32) - act64(pre64)| of the honest float32 model on the case's own inputs (case.delta;
    over the cases of the GPU test 1.2e-7 (one slab) to 1.7e-6 (eight) with ReLU and 3.3e-7 to 2.6e-6 with GELU, which puts at
    most 12 (bf16) / 54 (fp16) of a row's units next to a tie).  It stays at or below the old flat 2e-4 (fp16) / 2e-3 (bf16),
    asserted on every call; fp32 storage keeps the flat 1e-5."""
    inp = {"part": rnd((S, B, K), 1, 0.5), "b1": signed((K,), 2, 0.25, 0.5), "w": signed((2, K), 3, 0.02, 0.05),
           "b": signed((2,), 4, 0.1, 0.3)}

    def hidden64(i, slabs=S, noact_k=None):
        d = _d(i)
        pre = d["part"][:slabs].sum(0) + d["b1"]
        h = _act64(pre, act, noact_k)
        return h if dtype == F32 else h.to(dtype).double()

    def ref(i, last_from_prev=False, **kw):
        y = hidden64(i, **kw) @ i["w"].double().t() + i["b"].double()
        if last_from_prev:
            y = y.clone()
            y[B - 1] = y[B - 2]
        return y

    def act32(i):
        pre = i["part"].sum(0) + i["b1"]
        return {1: F.relu, 2: F.gelu}[act](pre)

    def model(i):
        h = act32(i)
        return ((h if dtype == F32 else q(h, dtype)) @ i["w"].t() + i["b"]).double()

    d = _d(inp)
    exact = _act64(d["part"].sum(0) + d["b1"], act)
    delta = 4.0 * (act32(inp).double() - exact).abs().max().item()
    bound = None
    if dtype != F32:
        near = ((_tie_distance(exact, dtype) <= delta) & (exact != 0)).double()
        bound = 1e-5 + (near * numutil.ulp(exact, dtype)) @ inp["w"].double().abs().t()

    defects = {}
    _head_defects(defects, inp, ref, B, K)
    for name, v in vec_variants(inp["b1"]).items():
        defects[f"b1_{name}"] = (lambda i, v=v: ref(_with(i, b1=v)))
    defects["last_slab_dropped"] = lambda i: ref(i, slabs=S - 1)
    defects["act_omitted_on_one_hidden_unit"] = lambda i: ref(i, noact_k=int(inp["b1"].argmin()))
    case = Case("head_tail_splitk", dtype, inp, ref, model, defects, 1.0, flat=HEAD_SPLITK_BEFORE[dtype], bound=bound,
                what=f"head_tail_splitk B={B} K={K} S={S} act={act}")
    case.delta, case.near_tie = delta, (0 if bound is None else int(near.sum(1).max().item()))
    return case


# msepart and mse are fp32 sums of squares: 3 x the largest relative error of the honest float32 model against the float64
# reference on resize_mse's inputs (B = 2; the largest of the three storage dtypes), floored at FP32_ACC.  Measured:
# msepart 1.7e-7, mse 1.0e-7 (x 3 below the floor), so both take the floor; the test this replaces allowed mse 1e-4 of its largest value.
MSE_REL = {"msepart": FP32_ACC, "mse": FP32_ACC}
MSE_REL_BEFORE = 1e-4


def _bilinear_x2(x, align_corners=False, wrap_right=False, wrap_bottom=False, swap_l=False):
    """(B, 3, 112, 112) -> (B, 3, 224, 224) in x's own precision: half-pixel source coordinates clamped below at 0, the
    second tap's index clamped at 111, the lerp in the kernel's order"""
    o = torch.arange(224, dtype=x.dtype)
    s = o * (111.0 / 223.0) if align_corners else ((o + 0.5) * 0.5 - 0.5).clamp(min=0)
    i0 = s.floor().long().clamp(max=111)
    frac = s - i0
    i1 = (i0 + 1).clamp(max=111)
    wrapped = torch.where(i0 + 1 > 111, torch.zeros_like(i0), i0 + 1)
    y0, y1 = i0[:, None], (wrapped if wrap_bottom else i1)[:, None]
    x0, x1 = i0[None, :], (wrapped if wrap_right else i1)[None, :]
    ly, lx = (frac[None, :], frac[:, None]) if swap_l else (frac[:, None], frac[None, :])
    v00, v01, v10, v11 = x[:, :, y0, x0], x[:, :, y0, x1], x[:, :, y1, x0], x[:, :, y1, x1]
    top, bot = v00 + (v01 - v00) * lx, v10 + (v11 - v10) * lx
    return top + (bot - top) * ly


def resize_mse(B, dtype):
    """bilinear 112 -> 224 (half-pixel, indices clamped) of x_hat and the per-frame MSE against img (gcv_k_resize_mse).  x_hat NCHW
    here (the test uploads NHWC).  Outputs: recon (B, 3, 224, 224) in the storage dtype; msepart (B, 196), the sum of
    (recon - img)^2 over the three channels of each block of 256 pixels, taken on the unrounded recon; mse (B,) their sum
    / (3 224 224)."""
    inp = {"xhat": q(rnd((B, 3, 112, 112), 1, 2.0), dtype), "img": q(rnd((B, 3, 224, 224), 2, 2.0), dtype)}
    count = 3.0 * 224 * 224

    def outputs(v, img, mse_count=count, blocks=196, last_from_prev=False):
        if last_from_prev:
            v = v.clone()
            v[B - 1] = v[B - 2]
        part = ((v - img) ** 2).sum(1).reshape(B, 196, 256).sum(2)
        return {"recon": v, "msepart": part, "mse": part[:, :blocks].sum(1) / mse_count}

    def ref(i, swap_channels=False, transposed=False, out_kw=None, **kw):
        d = _d(i)
        v = _bilinear_x2(d["xhat"], **kw)
        if swap_channels:
            v = v.flip(1)
        if transposed:
            v = v.transpose(2, 3)
        return outputs(v, d["img"], **(out_kw or {}))

    def model(i):
        o = outputs(_bilinear_x2(i["xhat"]), i["img"])
        return {"recon": _out(o["recon"], dtype), "msepart": o["msepart"].double(), "mse": o["mse"].double()}

    defects = {
        "align_corners": lambda i: ref(i, align_corners=True),
        "right_clamp_wraps_to_column_0": lambda i: ref(i, wrap_right=True),
        "bottom_clamp_wraps_to_row_0": lambda i: ref(i, wrap_bottom=True),
        "lx_ly_swapped": lambda i: ref(i, swap_l=True),
        "channels_0_and_2_swapped": lambda i: ref(i, swap_channels=True),
        "output_transposed": lambda i: ref(i, transposed=True),
        "mse_divided_by_224_224": lambda i: ref(i, out_kw={"mse_count": 224.0 * 224}),
        "last_block_left_out_of_mse": lambda i: ref(i, out_kw={"blocks": 195}),
    }
    if B > 1:
        defects["last_frame_from_frame_before"] = lambda i: ref(i, out_kw={"last_from_prev": True})
    what = f"resize_mse B={B}"
    case = MultiCase(what, dtype, inp, ref, model, defects, None)
    want = case.want()
    case.parts = {"recon": Case("resize", dtype, inp, None, None, None, 3.0, what=what + " recon")}
    for name in ("msepart", "mse"):
        case.parts[name] = Case("resize", dtype, inp, None, None, None, 1.0, what=f"{what} {name}",
                                flat=MSE_REL_BEFORE * want[name].abs().max().item(), bound=MSE_REL[name] * want[name].abs())
    return case


# ----------------------------------------------------------------------------- Swin-T kernels
SWIN_SENTINEL = 7.0      # what the GPU tests fill every output buffer with; a defect that leaves an element unwritten leaves this


def swin_rel_index():
    """row of the (169, nH) table for each (query, key) of a 7 x 7 window: (ty - jy + 6) 13 + (tx - jx + 6); (49, 49)"""
    t = torch.arange(49)
    dy, dx = t[:, None] // 7 - t[None, :] // 7, t[:, None] % 7 - t[None, :] % 7
    return (dy + 6) * 13 + (dx + 6)


def _swin_axis_regions(n, shift):
    """region id along one axis of the rolled map, from timm's three slices (0, -7), (-7, -shift), (-shift, end)"""
    lab = torch.zeros(n, dtype=torch.long)
    for cnt, s in enumerate((slice(0, -7), slice(-7, -shift), slice(-shift, None))):
        lab[s] = cnt
    return lab


def _swin_axis_regions_by_compare(n, size, edge):
    """the same by the kernels' comparisons, with the size the thresholds are taken from and the second edge as parameters
    (the defects): 0 below size - 7, 1 below edge, else 2"""
    c = torch.arange(n)
    return (c >= size - 7).long() + (c >= edge).long() * (c >= size - 7).long()


def _swin_windows(t, B, H, W):
    """(B, H, W, ch) -> (B nWy nWx, 49, ch), windows row-major"""
    return t.reshape(B, H // 7, 7, W // 7, 7, -1).permute(0, 1, 3, 2, 4, 5).reshape(B * (H // 7) * (W // 7), 49, -1)


def _swin_unwindow(t, B, H, W):
    return t.reshape(B, H // 7, W // 7, 7, 7, -1).permute(0, 1, 3, 2, 4, 5).reshape(B, H, W, -1)


def swin_attn_mask(H, W, shift, ly=None, lx=None, value=-100.0):
    """(nW, 49, 49): `value` between tokens of different regions of the rolled map, else 0"""
    ly = _swin_axis_regions(H, shift) if ly is None else ly
    lx = _swin_axis_regions(W, shift) if lx is None else lx
    mw = _swin_windows((ly[:, None] * 3 + lx[None, :]).reshape(1, H, W, 1), 1, H, W).reshape(-1, 49)
    differ = mw[:, :, None] != mw[:, None, :]
    return torch.where(differ, torch.full((), value, dtype=torch.float64), torch.zeros((), dtype=torch.float64))


_SWIN_UPPER = (torch.arange(49) & 4) != 0       # keys the MFMA kernel keeps on its upper lane half: kj = .. + 4 lh
_SWIN_PV_SWAP = torch.tensor([j + 4 if 4 <= j % 16 < 8 else (j - 4 if 8 <= j % 16 < 12 else j) for j in range(49)])


def _swin_variant_inputs(inp, variant, B, H, W, C, nH, shift):
    """the off-distribution inputs of tests/test_numerics_*: built in the rolled frame, where a token's place in its window
    is fixed, and rolled back"""
    qkv = inp["qkv"].clone()
    if variant == "uniform":                    # every unmasked logit 0: a row is the plain mean of its region's V rows
        qkv[..., :C] = 0
        return {"qkv": qkv, "table": torch.zeros_like(inp["table"])}
    j = (torch.arange(H)[:, None] % 7) * 7 + torch.arange(W)[None, :] % 7          # place in the window, rolled frame
    if variant == "wide":
        # channel 0 of each head: key j holds a ramp 32 .. -22 over a seeded order of the keys whose top key is on the upper
        # lane half and whose bottom key on the lower; query j holds +17 (even j) or -17.  Logits 0.177 x 17 x (32 .. -22) = 96
        # .. -66 for the even queries (exp(96) overflows fp32) and 66 .. -96 for the odd: a span of 162 with the largest
        # magnitude kept near the 89 an overflow needs.  The other 31 channels of q are zero: each of 31 additions to a partial
        # sum of magnitude 96 rounds at its spacing of 7.6e-6, two keys of a row that the mask brings within 1 of each other
        # turn a logit error d into 0.25 d |v1 - v2|, and with random channels the honest float32 model alone came to 3.0e-5 of
        # fp32 storage's 4e-5.  With one product per logit it stays below 1e-5; the contraction is the benign cases' subject
        order = torch.randperm(49, generator=torch.Generator().manual_seed(5)).tolist()
        top = next(k for k in order if k & 4)
        order.remove(top)
        bottom = next(k for k in reversed(order) if not k & 4)
        order.remove(bottom)
        order = [top] + order + [bottom]
        ramp = torch.empty(49)
        ramp[torch.tensor(order)] = 32.0 - 54.0 * torch.arange(49) / 48.0
        q0, k0 = torch.where(j % 2 == 0, 17.0, -17.0), ramp[j]
        qkv[..., :C] = 0
    else:                                       # "mask100": the last key of every window leads the others by 0.177 x 16 x 42.5 = 120
        q0, k0 = torch.full((H, W), 16.0), torch.where(j == 48, 42.5, 0.0)
    q0, k0 = (torch.roll(t, shifts=(shift, shift), dims=(0, 1)) for t in (q0, k0))
    for h in range(nH):
        qkv[..., h * 32] = q0
        qkv[..., C + h * 32] = k0
    return {"qkv": qkv, "table": inp["table"]}


def swin_attn(B, H, W, C, nH, shift, dtype, qk_scale=1.5, variant="benign"):
    """W-MSA / SW-MSA of timm 0.6.5 on a (B, H, W, 3C) qkv tensor, head_dim 32, for any H x W that 7 divides
    (gcv_k_swin_window_attn): roll by -shift, 7 x 7 windows, softmax(q k^T 32^-0.5 + table[index] + mask) v, windows back,
    roll by +shift.  q, k and v are U(-1.5, 1.5) (q and k times qk_scale / 1.5).  The table is +-[0.5, 1], rows 0 and 168
    +[0.5, 1]: each of the two is reached by one (query, key) pair of a window, whose probability p a zeroed entry t moves by
    p (1 - e^-t) where t > 0 and by e^t times less where t < 0.  At one window and one head that single pair has to show: in bf16
    +-[0.25, 0.5] left row 168 at 1.3 x the bound there, this at 4.3 x.  Where the shift mask splits every window along an axis
    (shift != 0 and a single window row or column) the two corner pairs are masked in every window, and zeroing them moves
    nothing: those two defects are left out there.
    The model rounds the unnormalised probabilities exp(s - max) to a 16-bit storage dtype in front of P.V and divides by
    the fp32 sum of the unrounded ones, as swin_window_attn_mfma_kernel does.  `variant`: the inputs of the softmax cases
    of tests/test_numerics_* ("uniform", "wide", "mask100") with their own defects; case.logits() are the float64 logits
    with bias and mask (mask=False: without), (B nW, nH, 49, 49)."""
    nWy, nWx = H // 7, W // 7
    nW = nWy * nWx
    qkv = rnd((B, H, W, 3 * C), 1, 1.5)
    qkv[..., :2 * C] *= qk_scale / 1.5
    table = signed((169, nH), 2, 0.5, 1.0)
    table[[0, 168]] = table[[0, 168]].abs()
    inp = {"qkv": q(qkv, dtype), "table": table}
    if variant != "benign":
        inp = _swin_variant_inputs(inp, variant, B, H, W, C, nH, shift)
        inp["qkv"] = q(inp["qkv"], dtype)
    index = swin_rel_index()
    if shift:
        for n in (H, W):
            assert torch.equal(_swin_axis_regions(n, shift), _swin_axis_regions_by_compare(n, n, n - shift))

    def logits(i, f=torch.float64, index=index, use_scale=True, mask=None):
        x = i["qkv"].to(f)
        if shift:
            x = torch.roll(x, shifts=(-shift, -shift), dims=(1, 2))
        qq, kk, vv = _swin_windows(x, B, H, W).reshape(B * nW, 49, 3, nH, 32).permute(2, 0, 3, 1, 4).unbind(0)
        s = (qq * 32 ** -0.5 if use_scale else qq) @ kk.transpose(-2, -1)
        s = s + i["table"].to(f)[index.reshape(-1)].reshape(49, 49, nH).permute(2, 0, 1)
        if shift and mask is not False:
            m = (swin_attn_mask(H, W, shift) if mask is None else mask).to(f)
            s = (s.reshape(B, nW, nH, 49, 49) + m[None, :, None]).reshape(B * nW, nH, 49, 49)
        return s, vv

    def attend(s, vv, f, p_dtype=None, pad_keys=False, lower_half_sum=False, pv_swap=False, half_max=False, no_max=False):
        if no_max:
            mx = torch.zeros_like(s[..., :1])
        elif half_max:
            up = _SWIN_UPPER.expand_as(s)
            ninf = torch.full_like(s, -math.inf)
            mx = torch.where(up, torch.where(up, s, ninf).amax(-1, keepdim=True), torch.where(up, ninf, s).amax(-1, keepdim=True))
        else:
            mx = s.amax(-1, keepdim=True)
            if pad_keys:
                mx = mx.clamp(min=0)
        p = torch.exp(s - mx)
        den = (p[..., ~_SWIN_UPPER] if lower_half_sum else p).sum(-1, keepdim=True)
        if pad_keys:
            den = den + 15.0 * torch.exp(-mx)
        if p_dtype is not None:
            p = p.to(p_dtype).to(f)
        pv = p @ (vv[..., _SWIN_PV_SWAP, :] if pv_swap else vv)
        return pv / den if f == torch.float64 else pv * (1.0 / den)

    def place(o, unroll=True, last_window_prev=False, last_image_prev=False, covered=None):
        o = o.transpose(1, 2).reshape(B * nW, 49, C)
        if last_window_prev:
            o = o.clone()
            o[-1] = o[-2]
        if covered is not None:
            o = o.clone().reshape(B, nW, 49, C)
            o[:, [w for w in range(nW) if w not in covered]] = SWIN_SENTINEL
        o = _swin_unwindow(o, B, H, W)
        if shift and unroll:
            o = torch.roll(o, shifts=(shift, shift), dims=(1, 2))
        if last_image_prev:
            o = o.clone()
            o[B - 1] = o[B - 2]
        return o.contiguous()

    def ref(i, lkw=None, akw=None, pkw=None):
        s, vv = logits(i, **(lkw or {}))
        return place(attend(s, vv, torch.float64, **(akw or {})), **(pkw or {}))

    def model(i):
        s, vv = logits(i, torch.float32)
        return _out(place(attend(s, vv, torch.float32, p_dtype=None if dtype == F32 else dtype)), dtype)

    def no_max_fp32(i):
        s, vv = logits(i, torch.float32)                    # exp(136) is finite in float64: the defect shows in the kernel's fp32
        return place(attend(s, vv, torch.float32, no_max=True)).double()

    def table_row_zeroed(r):
        def f(i):
            t = i["table"].clone()
            t[r] = 0
            return ref(_with(i, table=t))
        return f

    t49 = torch.arange(49)
    dy, dx = t49[:, None] // 7 - t49[None, :] // 7, t49[:, None] % 7 - t49[None, :] % 7
    if variant == "uniform":
        defects = {"padded_keys_in_the_softmax_sum": lambda i: ref(i, akw={"pad_keys": True})}
    elif variant == "wide":
        defects = {"max_taken_per_lane_half": lambda i: ref(i, akw={"half_max": True}), "max_not_subtracted": no_max_fp32}
    elif variant == "mask100":
        defects = {"mask_is_minus_inf": lambda i: ref(i, lkw={"mask": swin_attn_mask(H, W, shift, value=-math.inf)})}
    else:
        corners_seen = not shift or (nWy > 1 and nWx > 1)
        defects = {f"table_row_{r}_zeroed": table_row_zeroed(r) for r in (0, 168, 84) if r == 84 or corners_seen}
        if nH > 1:
            defects["table_column_of_next_head"] = lambda i: ref(_with(i, table=torch.roll(i["table"], -1, dims=1)))
        defects["rel_index_transposed"] = lambda i: ref(i, lkw={"index": (dx + 6) * 13 + (dy + 6)})
        defects["rel_index_negated"] = lambda i: ref(i, lkw={"index": (6 - dy) * 13 + (6 - dx)})
        defects["scale_omitted"] = lambda i: ref(i, lkw={"use_scale": False})
        if shift:
            defects["shift_mask_omitted"] = lambda i: ref(i, lkw={"mask": False})
            if H != W:
                lx_h = _swin_axis_regions_by_compare(W, H, H - shift)
                defects["mask_regions_with_H_on_both_axes"] = lambda i: ref(i, lkw={"mask": swin_attn_mask(H, W, shift, lx=lx_h)})
            ly_1 = _swin_axis_regions_by_compare(H, H, H - shift - 1)
            defects["region_edge_off_by_one"] = lambda i: ref(i, lkw={"mask": swin_attn_mask(H, W, shift, ly=ly_1)})
            defects["reverse_roll_omitted"] = lambda i: ref(i, pkw={"unroll": False})
        if H != W:
            # wy = win / nWy, wx = win - wy nWy: some windows are computed twice (the kernels wrap coordinates into the map),
            # the others never: those keep what the buffer held
            covered = {((w // nWy) % nWy) * nWx + (w - (w // nWy) * nWy) % nWx for w in range(nW)}
            assert len(covered) < nW
            defects["window_index_decomposed_with_nWy"] = lambda i: ref(i, pkw={"covered": covered})
        defects["padded_keys_in_the_softmax_sum"] = lambda i: ref(i, akw={"pad_keys": True})
        defects["normaliser_over_one_lane_half"] = lambda i: ref(i, akw={"lower_half_sum": True})
        defects["pv_keys_4_7_and_8_11_exchanged"] = lambda i: ref(i, akw={"pv_swap": True})
        if B * nW > 1:
            defects["last_window_from_window_before"] = lambda i: ref(i, pkw={"last_window_prev": True})
        if B > 1:
            defects["last_image_from_image_before"] = lambda i: ref(i, pkw={"last_image_prev": True})
    case = Case("swin_attn", dtype, inp, ref, model, defects, 2.0,
                what=f"swin_attn B={B} {H}x{W} C={C} nH={nH} shift={shift}" + ("" if variant == "benign" else f" {variant}"))
    case.logits = lambda **kw: logits(inp, **kw)[0]
    return case


def patch_merge_ln(C, H, W, n, dtype):
    """Swin PatchMerging's front half (gcv_k_patch_merge_ln): LayerNorm(4C, eps 1e-5) over timm's concat
    [x(0::2, 0::2), x(1::2, 0::2), x(0::2, 1::2), x(1::2, 1::2)]; x (n, H, W, C) -> (n, H / 2, W / 2, 4C)"""
    inp = {"x": q(rnd((n, H, W, C), 1, 2.0), dtype), "lw": signed((4 * C,), 4, 0.5, 1.5), "lb": signed((4 * C,), 5, 0.1, 0.3)}

    def gather(x, patchify_order=False, stride_h=False):
        if stride_h:                      # pixel (b, y, xx) read at ((b H + y) H + xx) C of the buffer
            b, y, xx = torch.meshgrid(torch.arange(n), torch.arange(H), torch.arange(W), indexing="ij")
            x = x.reshape(n * H * W, C)[((b * H + y) * H + xx) % (n * H * W)]
        parts = [x[:, 0::2, 0::2], x[:, 1::2, 0::2], x[:, 0::2, 1::2], x[:, 1::2, 1::2]]
        if patchify_order:
            parts = [parts[0], parts[2], parts[1], parts[3]]
        return torch.cat(parts, -1)

    def ref(i, first_quadrant_stats=False, last_from_prev=False, **kw):
        d = _d(i)
        r = gather(d["x"], **kw)
        if first_quadrant_stats:
            mean = r[..., :C].mean(-1, keepdim=True)
            var = ((r[..., :C] - mean) ** 2).mean(-1, keepdim=True)
            y = (r - mean) / torch.sqrt(var + 1e-5) * d["lw"] + d["lb"]
        else:
            y = numutil.ln_ref(r, d["lw"], d["lb"], 1e-5)
        return _last_from_prev(y) if last_from_prev else y.contiguous()

    def model(i):
        return _out(F.layer_norm(gather(i["x"]), (4 * C,), i["lw"], i["lb"], 1e-5), dtype)

    defects = {}
    _vec_defects(defects, inp, ref, ("lw", "lb"))
    defects["quadrants_dy_dx_swapped"] = lambda i: ref(i, patchify_order=True)
    if H != W:
        defects["rows_strided_by_H"] = lambda i: ref(i, stride_h=True)
    defects["statistics_over_the_first_quadrant"] = lambda i: ref(i, first_quadrant_stats=True)
    if n * (H // 2) * (W // 2) > 1:
        defects["last_row_from_row_before"] = lambda i: ref(i, last_from_prev=True)
    return Case("patch_merge_ln", dtype, inp, ref, model, defects, 3.0, what=f"patch_merge_ln C={C} {H}x{W} n={n}")


def mean_tokens(n, L, C, dtype):
    """mean over the L tokens of each image (gcv_k_mean_tokens): x (n, L, C) -> (n, C)"""
    inp = {"x": q(rnd((n, L, C), 1, 2.0), dtype)}

    def ref(i, drop_last=False, div_plus_1=False, last_from_prev=False, last_channel_unwritten=False):
        x = i["x"].double()
        m = (x[:, :L - 1] if drop_last else x).sum(1) / ((L + 1) if div_plus_1 else L)
        if last_from_prev:
            m = m.clone()
            m[n - 1] = m[n - 2]
        if last_channel_unwritten:
            m = m.clone()
            m[:, C - 1] = SWIN_SENTINEL
        return m

    def model(i):
        return _out(i["x"].mean(1), dtype)

    defects = {"mean_divided_by_L_plus_1": lambda i: ref(i, div_plus_1=True)}
    if L > 1:
        defects["last_token_left_out_of_the_mean"] = lambda i: ref(i, drop_last=True)
    if n > 1:
        defects["last_image_from_image_before"] = lambda i: ref(i, last_from_prev=True)
    if C % 256:
        defects["last_channel_of_a_partly_filled_trip_unwritten"] = lambda i: ref(i, last_channel_unwritten=True)
    return Case("mean_tokens", dtype, inp, ref, model, defects, 1.0, what=f"mean_tokens n={n} L={L} C={C}")


def layernorm_rows(rows, C, dtype):
    """LayerNorm(C, eps 1e-5) of each row (gcv_k_layernorm_rows), any C <= 1536.  Each row carries an offset of +-[0.5, 1]:
    lanes past C that were counted in the variance as (0 - mean)^2 show only on a row whose mean is not near zero."""
    inp = {"x": q(rnd((rows, C), 1, 2.0) + signed((rows, 1), 6, 0.5, 1.0), dtype), "lw": signed((C,), 4, 0.5, 1.5),
           "lb": signed((C,), 5, 0.1, 0.3)}
    Cp = 64 * -(-C // 64)

    def ref(i, last_from_prev=False, padded_width=False, padded_lanes_in_variance=False):
        d = _d(i)
        x = d["x"]
        n = Cp if padded_width else C
        mean = x.sum(-1, keepdim=True) / n
        var = ((x - mean) ** 2).sum(-1, keepdim=True)
        if padded_lanes_in_variance:
            var = var + (Cp - C) * mean ** 2
        y = (x - mean) / torch.sqrt(var / n + 1e-5) * d["lw"] + d["lb"]
        if last_from_prev:
            y = y.clone()
            y[rows - 1] = y[rows - 2]
        return y

    def model(i):
        return _out(F.layer_norm(i["x"], (C,), i["lw"], i["lb"], 1e-5), dtype)

    defects = {}
    _vec_defects(defects, inp, ref, ("lw", "lb"))
    if rows > 1:
        defects["last_row_from_row_before"] = lambda i: ref(i, last_from_prev=True)
    if C % 64:
        defects["statistics_divided_by_the_padded_width"] = lambda i: ref(i, padded_width=True)
        defects["padded_lanes_counted_in_the_variance"] = lambda i: ref(i, padded_lanes_in_variance=True)
    return Case("layernorm_rows", dtype, inp, ref, model, defects, 3.0, what=f"layernorm_rows rows={rows} C={C}")
