"""Per-kernel parity on the MI355X: every HIP kernel (called through the C ABI's gcv_k_* entry
points) against a plain PyTorch fp32 CPU reference of the same op.  fp32 storage must agree to
~1e-5; 16-bit storage is checked against the same fp32 math on inputs rounded to that dtype.
The families that feed the verdict (fused MLPs, the GEMM epilogues, conv-as-GEMM, dw7x7 + LN, and the small kernels between a
frame and the two logits: stem, LN-patchify, pool + LN, first conv, last convT, reparam, head tail, resize + MSE) take inputs,
float64 reference and per-element comparator from tests/kcases.py; tests/test_kernel_sensitivity_cpu.py shows, without a GPU,
which planted defects that comparator rejects.  Where a case is meant for one kernel of a launcher, the test asserts the
launcher's own rule on the pointers, strides and shape it passes.  The Swin-T kernels (window attention, patch merging, token
mean, layernorm_rows) are on the same builders.  The Grad-CAM backward kernels are on builders of the same kind in
tests/camcases.py; their per-kernel tests are tests/test_cam_kernels_gpu.py."""
import ctypes
import math

import pytest
import torch
import torch.nn.functional as F

from genconvit_amd import _lib
from tests import dwcases, gemmcases, kcases, kutil
from tests.kutil import DTYPES, dev, gemm, ptr, rnd, tol

pytestmark = pytest.mark.gpu
torch.set_grad_enabled(False)

ALL = ["f32", "bf16", "f16"]


_KEEP = []


def D(t, dtype=None):
    """device copy that stays alive for the duration of the test (the caching allocator would
    otherwise hand a freed temporary's block to the next one before the kernel has run)"""
    d = t.to(dev()) if dtype is None else t.to(dev(), dtype)
    _KEEP.append(d)
    if len(_KEEP) > 64:
        torch.cuda.synchronize()
        del _KEEP[:32]
    return d


def q(t, dtype):
    """round a fp32 CPU tensor through the storage dtype"""
    return t.to(dtype).float()


def act_ref(x, act):
    return {0: lambda v: v, 1: F.relu, 2: F.gelu, 3: lambda v: F.leaky_relu(v, 0.01)}[act](x)


def assert_close(got, want, atol, what=""):
    err = (got.float().cpu() - want).abs().max().item()
    assert err <= atol, f"{what}: max abs err {err:.3e} > {atol:.3e}"


# ----------------------------------------------------------------------------- GEMM, plain A
@pytest.mark.parametrize("dt", ALL)
@pytest.mark.parametrize("M,N,K,act", gemmcases.cases(gemmcases.BIAS_ACT))
def test_gemm_bias_act(dt, M, N, K, act):
    dtype = DTYPES[dt]
    case = kcases.gemm("bias_act", M, N, K, dtype, act=act)
    i = case.inputs
    ldc = N + 8
    C = torch.full((M, ldc), 7.0, dtype=dtype, device=dev())
    gemm(dtype, _lib.A_PLAIN, _lib.EPI_BIAS_ACT, D(i["A"], dtype), D(i["W"], dtype), C, M, N, K, lda=K, ldc=ldc,
         bias=D(i["bias"]), act=act)
    assert torch.all(C[:, N:].float() == 7.0), "padding columns were overwritten"
    case.assert_close(C[:, :N])


@pytest.mark.parametrize("dt", ALL)
def test_gelu_nan_behaviour_is_documented(dt):
    """A NaN pre-activation (here: injected through the bias) in the GELU epilogue.  fp32 storage (exact erf, float max)
    propagates every NaN.  The 16-bit paths take max(x, 0) as an integer max of the bit pattern (csrc/gemm.h GeluH16): a
    NaN with a clear sign bit still propagates, one with the sign bit set comes out as a finite number — accepted and
    documented there; this test pins that behaviour so that a change of it is a decision."""
    dtype = DTYPES[dt]
    M, N, K = 300, 384, 96
    A, W = q(rnd((M, K), 1), dtype), q(rnd((N, K), 2, 1 / math.sqrt(K)), dtype)
    bias = rnd((N,), 3, 0.1)
    bias[5] = float("nan")
    bias[7] = torch.tensor([0xFFC00000 - (1 << 32)], dtype=torch.int32).view(torch.float32)[0]   # NaN, sign bit set
    C = torch.zeros((M, N), dtype=dtype, device=dev())
    gemm(dtype, _lib.A_PLAIN, _lib.EPI_BIAS_ACT, D(A, dtype), D(W, dtype), C, M, N, K, lda=K, ldc=N, bias=D(bias), act=2)
    out = C.float().cpu()
    clean = [c for c in range(N) if c not in (5, 7)]
    assert torch.isfinite(out[:, clean]).all()
    assert torch.isnan(out[:, 5]).all(), "a positive NaN must propagate in every dtype"
    if dtype == torch.float32:
        assert torch.isnan(out[:, 7]).all(), "fp32 storage propagates every NaN"
    else:
        assert torch.isfinite(out[:, 7]).all(), "documented: sign-bit NaN -> finite in the packed 16-bit GELU"


@pytest.mark.parametrize("dt", ALL)
@pytest.mark.parametrize("M,N,K", gemmcases.cases(gemmcases.RESID))
def test_gemm_layerscale_residual(dt, M, N, K):
    _resid_case(DTYPES[dt], M, N, K)


def _resid_case(dtype, M, N, K):
    case = kcases.gemm("resid", M, N, K, dtype)
    i = case.inputs
    Xd = D(i["X"], dtype).clone()
    gemm(dtype, _lib.A_PLAIN, _lib.EPI_RESID, D(i["A"], dtype), D(i["W"], dtype), Xd, M, N, K, lda=K, ldc=N,
         bias=D(i["bias"]), gamma=D(i["gamma"]), resid=Xd)              # in place, like the forward does
    case.assert_close(Xd)


@pytest.mark.parametrize("dt", ALL)
@pytest.mark.parametrize("M,N,K,splitk,kps", gemmcases.cases(gemmcases.SPLITK))
def test_gemm_splitk(dt, M, N, K, splitk, kps):
    dtype = DTYPES[dt]
    case = kcases.gemm("splitk", M, N, K, dtype, k_per_split=kps)
    i = case.inputs
    part = torch.zeros((splitk, M, N), dtype=torch.float32, device=dev())
    gemm(dtype, _lib.A_PLAIN, _lib.EPI_SPLITK, D(i["A"], dtype), D(i["W"], dtype), None, M, N, K, lda=K,
         partial=part, splitk=splitk, k_per_split=kps)
    case.assert_close(part.sum(0))


# ----------------------------------------------------------------------------- conv as GEMM
@pytest.mark.parametrize("dt", ALL)
@pytest.mark.parametrize("n,H,cin,cout", gemmcases.cases(gemmcases.CONV_POOL))
def test_conv3x3_relu_maxpool(dt, n, H, cin, cout):
    """ED encoder layers 2-5 (model/genconvit_ed.py:18-32): conv3x3 s1 p1 -> ReLU -> maxpool2."""
    dtype = DTYPES[dt]
    case = kcases.conv3x3_pool(n, H, cin, cout, dtype)
    x, w, b = (case.inputs[k] for k in ("x", "w", "b"))
    x_nhwc = D(x.permute(0, 2, 3, 1).contiguous(), dtype)
    wt = D(w.permute(0, 2, 3, 1).reshape(cout, 9 * cin).contiguous(), dtype)
    out = torch.zeros((n, H // 2, H // 2, cout), dtype=dtype, device=dev())
    gemm(dtype, _lib.A_IM2COL3_POOL, _lib.EPI_POOL4, x_nhwc, wt, out, n * H * H, cout, 9 * cin, ldc=cout,
         bias=D(b), act=1, H=H, W=H, cin_log2=int(math.log2(cin)))
    case.assert_close(out)


@pytest.mark.parametrize("dt", ALL)
@pytest.mark.parametrize("n,H,cin,cout", gemmcases.cases(gemmcases.CONV_S2))
def test_conv3x3_stride2_leaky(dt, n, H, cin, cout):
    """VAE encoder layers 2-4 (model/genconvit_vae.py:19-30), BatchNorm folded by the caller."""
    dtype = DTYPES[dt]
    case = kcases.conv3x3_s2(n, H, cin, cout, dtype)
    x, w, b = (case.inputs[k] for k in ("x", "w", "b"))
    x_nhwc = D(x.permute(0, 2, 3, 1).contiguous(), dtype)
    wt = D(w.permute(0, 2, 3, 1).reshape(cout, 9 * cin).contiguous(), dtype)
    out = torch.zeros((n, H // 2, H // 2, cout), dtype=dtype, device=dev())
    gemm(dtype, _lib.A_IM2COL3_S2, _lib.EPI_BIAS_ACT, x_nhwc, wt, out, n * (H // 2) ** 2, cout, 9 * cin, ldc=cout,
         bias=D(b), act=3, H=H, W=H, cin_log2=int(math.log2(cin)))
    case.assert_close(out)


@pytest.mark.parametrize("dt", ALL)
@pytest.mark.parametrize("n,H,cin,cout,act", gemmcases.cases(gemmcases.CONV_T))
def test_conv_transpose_2x2(dt, n, H, cin, cout, act):
    """ED / VAE decoder ConvTranspose2d(k=2,s=2) layers (genconvit_ed.py:44-55, genconvit_vae.py:68-76)."""
    dtype = DTYPES[dt]
    case = kcases.conv_transpose2x2(n, H, cin, cout, act, dtype)
    x, w, b = (case.inputs[k] for k in ("x", "w", "b"))
    x_nhwc = D(x.permute(0, 2, 3, 1).contiguous(), dtype)
    wt = D(w.permute(2, 3, 1, 0).reshape(4 * cout, cin).contiguous(), dtype)           # ((dy,dx,co), ci)
    out = torch.zeros((n, 2 * H, 2 * H, cout), dtype=dtype, device=dev())
    gemm(dtype, _lib.A_PLAIN, _lib.EPI_CONVT, x_nhwc, wt, out, n * H * H, 4 * cout, cin, lda=cin, bias=D(b),
         act=act, H=H, W=H, cout_log2=int(math.log2(cout)))
    case.assert_close(out)


# ----------------------------------------------------------------------------- ConvNeXt pieces
H16 = ["bf16", "f16"]
SENT = 7.0


def _stem_takes_matrix_pipe(dtype, x_ptr, out_ptr, sb, sc, sy, sx, total):
    """launch_stem_ln_c's own test (csrc/kernels_impl.h): stem_ln_mfma_kernel for 16-bit storage, x 8-byte and `out` 16-byte
    aligned, sb and sy multiples of 4, and NCHW (sx = 1, sc a multiple of 4) or NHWC (sc = 1, sx = 3); else stem_ln_kernel"""
    if dtype == torch.float32:
        return False
    al = x_ptr % 8 == 0 and (sb | sy) % 4 == 0 and out_ptr % 16 == 0
    return al and ((sx == 1 and sc % 4 == 0) or (sc == 1 and sx == 3)) and total < 1 << 30


def _stem_case(dtype, C, n, Ho, Wo, layout, kernel, pad=0, xs=0, os_=0, entry="gcv_k_stem_ln_c"):
    """the stem on n frames of 4 Ho x 4 Wo against kcases.stem.  `pad`: the NCHW frames are cut out of a buffer whose rows are
    `pad` elements longer (filled with 3); xs / os_: x / out that many elements off their allocation's start.  `kernel`
    ("mfma" / "valu") is asserted by the launcher's own rule.  Sentinels in front of and behind the T tokens of `out`."""
    case = kcases.stem(C, n, Ho, Wo, layout, dtype)
    i = case.inputs
    H, W, T = 4 * Ho, 4 * Wo, n * Ho * Wo
    if layout == "nchw":
        frame = torch.full((n, 3, H, W + pad), 3.0)
        frame[..., :W] = i["x"]
        st = (3 * H * (W + pad), H * (W + pad), W + pad, 1)
    else:
        assert pad == 0
        frame, st = i["x"].permute(0, 2, 3, 1).contiguous(), (H * W * 3, 1, W * 3, 3)
    xbuf = torch.zeros((xs + frame.numel(),), dtype=dtype, device=dev())
    xbuf[xs:] = frame.reshape(-1).to(dev(), dtype)
    obuf = torch.full((os_ + (T + 8) * C,), SENT, dtype=dtype, device=dev())
    xd, out = xbuf[xs:], obuf[os_:]
    assert xd.data_ptr() % 8 == (xs * xd.element_size()) % 8 and out.data_ptr() % 16 == (os_ * out.element_size()) % 16
    takes = _stem_takes_matrix_pipe(dtype, xd.data_ptr(), out.data_ptr(), *st, T)
    assert takes == (kernel == "mfma"), f"this launch does not reach the {kernel} kernel"
    wp = D(i["w"].reshape(C, 48).t().contiguous())
    assert wp.data_ptr() % 16 == 0
    args = (_lib.dtype_code(dtype), ptr(xd), *st, ptr(wp), ptr(D(i["bias"])), ptr(D(i["lw"])), ptr(D(i["lb"])), ptr(out),
            n, Ho, Wo)
    if entry == "gcv_k_stem_ln":
        assert C == 96
        kutil.call(entry, *args, 1e-6)
    else:
        kutil.call(entry, *args, C, 1e-6)
    assert (obuf[:os_].float() == SENT).all() and (out[T * C:].float() == SENT).all(), "written outside the T tokens"
    case.assert_close(out[:T * C].reshape(T, C))


@pytest.mark.parametrize("dt", ALL)
@pytest.mark.parametrize("layout,res", [("nchw", 224), ("nhwc", 112), ("nchw", 32), ("nchw", 20), ("nhwc", 20)])   # 20: a 25-token tail tile
def test_stem_conv4x4_layernorm(dt, layout, res):
    dtype = DTYPES[dt]
    _stem_case(dtype, 96, 2, res // 4, res // 4, layout, "valu" if dtype == torch.float32 else "mfma", entry="gcv_k_stem_ln")


# (n, Ho, Wo, layout, pad): one token (every lane clamps to total - 1); 243 tokens (a ragged eighth tile, two workgroups);
# a non-square frame; NCHW frames cut out of a buffer 8 elements wider than the row (sy = W + 8, sc = H sy, sb = 3 sc)
_STEM_FRAMES = [(1, 1, 1, "nchw", 0), (1, 1, 1, "nhwc", 0), (3, 9, 9, "nchw", 0), (3, 9, 9, "nhwc", 0),
                (2, 5, 8, "nchw", 0), (2, 5, 8, "nhwc", 0), (2, 5, 8, "nchw", 8)]


@pytest.mark.parametrize("dt", H16)
@pytest.mark.parametrize("C", [96, 192])
@pytest.mark.parametrize("n,Ho,Wo,layout,pad", _STEM_FRAMES)
def test_stem_matrix_pipe_kernel(dt, C, n, Ho, Wo, layout, pad):
    """stem_ln_mfma_kernel<T, C / 32> at both widths and frame layouts"""
    _stem_case(DTYPES[dt], C, n, Ho, Wo, layout, "mfma", pad=pad)


def test_stem_matrix_pipe_kernel_second_trip_of_the_stride_loop():
    """One frame of 513 x 513 tokens: 8225 tiles of 32 tokens on the grid's 2048 x 4 = 8192 waves, so 33 waves take a second trip
    (the prefetch of tile + stride lands in a live tile) and the last tile is ragged (one token)."""
    _stem_case(torch.bfloat16, 96, 1, 513, 513, "nchw", "mfma")


@pytest.mark.parametrize("C", [96, 192])
@pytest.mark.parametrize("layout,pad", [("nchw", 0), ("nhwc", 0), ("nchw", 8)])
def test_stem_valu_kernel_fp32_off_square_and_strided_frames(C, layout, pad):
    """stem_ln_kernel<float, C> on the non-square frame and on the frame with a row stride larger than the row"""
    _stem_case(torch.float32, C, 2, 5, 8, layout, "valu", pad=pad)


@pytest.mark.parametrize("dt", ["bf16", "f16"])
@pytest.mark.parametrize("C", [96, 192])
@pytest.mark.parametrize("layout", ["nchw", "nhwc"])
@pytest.mark.parametrize("path", ["out+8B", "x+1elem"])
def test_stem_valu_kernel_in_16bit_storage(dt, C, layout, path):
    """stem_ln_kernel<T, C> in 16-bit storage, which aligned operands never reach (they take stem_ln_mfma_kernel):
    launch_stem_ln_c's `al` test sends a launch there when x is not 8-byte or `out` not 16-byte aligned.
      out+8B : `out` 8 bytes off a 16-byte boundary, x aligned -> the kernel's 8-byte patch staging (its own `al` looks at x
               and the strides only); the output is written one element at a time (`o[i] = from_f<T>(...)`).
      x+1elem: x one element off -> the per-element staging (`to_f(x[...])`); `out` aligned.
    res 36: 9 x 9 tokens per image, so the last workgroup's token tile is ragged.  Sentinels in front of and behind `out`."""
    xs, os_ = (0, 4) if path == "out+8B" else (1, 0)
    _stem_case(DTYPES[dt], C, 3, 9, 9, layout, "valu", xs=xs, os_=os_)


@pytest.mark.parametrize("dt", ALL)
@pytest.mark.parametrize("C,H,n", dwcases.SQUARE)
def test_dwconv7x7_layernorm(dt, C, H, n):
    """ConvNeXt block front half: depthwise 7x7 p3 + LayerNorm(C, eps 1e-6), NHWC."""
    _dw_case(DTYPES[dt], C, H, H, n)


def _dw_case(dtype, C, H, W, n, shift=0, plan_nimg=0):
    """gcv_k_dwconv7_ln on n maps of H x W x C against the float64 conv + LayerNorm of kcases.dwconv7_ln.  The output buffer
    is one image longer than the launch and pre-filled with a sentinel: nothing behind the last image — and, with `shift`
    elements of offset from the allocation's start, nothing in front of the first — may be written.  plan_nimg > 0:
    gcv_k_dwconv7_ln_planned, the n images under the kernel and the rows per band of a launch of plan_nimg images."""
    case = kcases.dwconv7_ln(C, H, W, n, dtype, aligned=shift == 0, plan_nimg=plan_nimg)
    x, w, b, lw, lb = (case.inputs[k] for k in ("x", "w", "b", "lw", "lb"))
    img = H * W * C
    xbuf = torch.zeros((shift + n * img,), dtype=dtype, device=dev())
    xbuf[shift:] = x.permute(0, 2, 3, 1).reshape(-1).to(dev(), dtype)
    ybuf = torch.full((shift + (n + 1) * img,), 7.0, dtype=dtype, device=dev())
    xd, out = xbuf[shift:], ybuf[shift:]
    assert xd.data_ptr() % 16 == (shift * xd.element_size()) % 16 and out.data_ptr() % 16 == xd.data_ptr() % 16
    wdw = w.reshape(C, 49).t().contiguous().to(dev())
    if plan_nimg > 0:
        kutil.call("gcv_k_dwconv7_ln_planned", _lib.dtype_code(dtype), ptr(xd), ptr(wdw), ptr(D(b)), ptr(D(lw)), ptr(D(lb)),
                   ptr(out), n, H, W, C, 1e-6, plan_nimg)
    else:
        kutil.call("gcv_k_dwconv7_ln", _lib.dtype_code(dtype), ptr(xd), ptr(wdw), ptr(D(b)), ptr(D(lw)), ptr(D(lb)), ptr(out),
                   n, H, W, C, 1e-6)
    assert (ybuf[:shift].float() == 7.0).all() and (out[n * img:].float() == 7.0).all(), "written outside the n images"
    case.assert_close(out[:n * img].reshape(n, H, W, C))


@pytest.mark.parametrize("dt", ALL)
@pytest.mark.parametrize("C,H,plan_nimg", dwcases.GEOMETRY)
def test_dwconv7x7_layernorm_at_every_band_geometry(dt, C, H, plan_nimg):
    """Two images under the plan of plan_nimg: every (kernel, H, rows per band) that a batch of ConvNeXt-T or ConvNeXt-L
    reaches in any network (tests/dwcases.py GEOMETRY; tests/test_host_cpu.py holds the list against the census of the
    networks' launches).  The bands of a large launch are long: the Roll walk's ring wraps, Pair reuses its double-buffered
    LayerNorm partials from row to row, Mfma runs whole-image bands."""
    _dw_case(DTYPES[dt], C, H, H, 2, plan_nimg=plan_nimg)


@pytest.mark.parametrize("dt", ALL)
@pytest.mark.parametrize("C,H,plan_nimg", dwcases.GEOMETRY_N3)
def test_dwconv7x7_layernorm_three_images_under_a_large_plan(dt, C, H, plan_nimg):
    """... and three images once per band kernel: an odd image count under the same plans"""
    _dw_case(DTYPES[dt], C, H, H, 3, plan_nimg=plan_nimg)


@pytest.mark.parametrize("dt", ALL)
@pytest.mark.parametrize("C,H,W,n", dwcases.TILE + dwcases.TILE_ODD)
def test_dwconv7x7_layernorm_tile_kernel(dt, C, H, W, n):
    """The generic tile kernel (dwconv7_ln_kernel<T, C>, DwKind::Tile) at each of its four widths: the maps of a res-160 pass
    (40 / 20 / 10 / 5), odd maps with ragged right and bottom tiles, non-square and single-row maps, and at C = 96 (two
    tiles per workgroup) odd tile counts, whose last workgroup has an idle second slot.  tests/test_host_cpu.py checks,
    without a GPU, that each of these shapes plans as Tile."""
    _dw_case(DTYPES[dt], C, H, W, n)


@pytest.mark.parametrize("dt", ALL)
def test_dwconv7x7_layernorm_unaligned_operands_run_the_tile_kernel(dt):
    """x and y one element off a 16-byte boundary: launch_dwconv7_ln tests (x | y) & 15 itself and sends the launch to Tile
    (dw_select: the band kernels are behind `if (aligned)`), whose every global access is one element wide — x through
    `rp[xoff[s]]`, y through `yb[...] = from_f<T>(...)`, the fp32 taps and LayerNorm vectors one float each
    (csrc/kernels_dev.h, dwconv7_ln_kernel).  56 x 56 at C = 96 is otherwise the Roll / Mfma shape."""
    _dw_case(DTYPES[dt], 96, 56, 56, 2, shift=1)


@pytest.mark.parametrize("dt", ALL)
@pytest.mark.parametrize("C,H,W,n", dwcases.BANDS)
def test_dwconv7x7_layernorm_band_kernels_off_square(dt, C, H, W, n):
    """The band kernels (Roll, Mfma in 16-bit storage, Pair) with H != W: a single row, fewer rows than the 7 taps, a height
    that is not a multiple of the band (57 rows: the last band is one row)."""
    _dw_case(DTYPES[dt], C, H, W, n)


def _lnp_case(dtype, C, H, W, n, kernel, shift=0):
    """gcv_k_ln_patchify against kcases.ln_patchify; x `shift` elements off its allocation's start.  `kernel` ("vec" /
    "generic") is asserted by launch_ln_patchify's own rule: ln_patchify_vec_kernel for 16-bit storage at C = 96 / 192 / 384
    with x and out 4-byte aligned.  One image of sentinel behind the output."""
    case = kcases.ln_patchify(C, H, W, n, dtype)
    i = case.inputs
    Ho, Wo = H // 2, W // 2
    xbuf = torch.zeros((shift + i["x"].numel(),), dtype=dtype, device=dev())
    xbuf[shift:] = i["x"].reshape(-1).to(dev(), dtype)
    out = torch.full((n + 1, Ho, Wo, 4 * C), SENT, dtype=dtype, device=dev())
    vec = dtype != torch.float32 and C in (96, 192, 384) and (xbuf[shift:].data_ptr() | out.data_ptr()) % 4 == 0
    assert vec == (kernel == "vec"), f"this launch does not reach the {kernel} kernel"
    kutil.call("gcv_k_ln_patchify", _lib.dtype_code(dtype), ptr(xbuf[shift:]), ptr(D(i["lw"])), ptr(D(i["lb"])), ptr(out),
               n, H, W, C, 1e-6)
    assert (out[n].float() == SENT).all(), "written beyond the last image"
    case.assert_close(out[:n])


@pytest.mark.parametrize("dt", ALL)
@pytest.mark.parametrize("C,H", [(96, 56), (192, 28), (384, 14), (384, 7), (192, 14)])
def test_layernorm2d_space_to_depth(dt, C, H):
    """Downsample front half: LayerNorm2d + 2x2 patch gather; odd sizes drop the last row/col (7 -> 3)."""
    dtype = DTYPES[dt]
    _lnp_case(dtype, C, H, H, 2, "generic" if dtype == torch.float32 else "vec")


@pytest.mark.parametrize("dt", H16)
@pytest.mark.parametrize("C,H,W,n", [(96, 3, 5, 1),       # 15 pixels: fewer than one block's 16
                                     (192, 2, 2, 1), (384, 7, 7, 2), (96, 6, 10, 3)])
def test_layernorm2d_space_to_depth_vector_kernel(dt, C, H, W, n):
    """ln_patchify_vec_kernel<T, C> at its three widths: less than one block, one patch row, odd and non-square maps"""
    _lnp_case(DTYPES[dt], C, H, W, n, "vec")


@pytest.mark.parametrize("dt", ALL)
@pytest.mark.parametrize("C,H,W", [(768, 14, 14), (768, 7, 7), (768, 5, 8), (192, 9, 9)])
def test_layernorm2d_space_to_depth_generic_kernel(dt, C, H, W):
    """ln_patchify_kernel<T> in every storage dtype: C = 768 (ConvNeXt-L's stage 2 -> 3 boundary) has no vectorised kernel,
    so 16-bit storage runs the generic one too.  Even and odd maps (last row / column dropped) and a non-square one."""
    dtype = DTYPES[dt]
    _lnp_case(dtype, C, H, W, 3, "generic" if (dtype == torch.float32 or C == 768) else "vec")


@pytest.mark.parametrize("dt", ["bf16", "f16"])
@pytest.mark.parametrize("H", [28, 7])
def test_layernorm2d_space_to_depth_2byte_aligned_input(dt, H):
    """16-bit storage at C = 96 with x two bytes off a 4-byte boundary: launch_ln_patchify's own `al` test ((x | out) & 3)
    skips ln_patchify_vec_kernel for the generic kernel, which reads `src[c]` and writes `dst[c]` one element at a time
    (csrc/kernels_dev.h, ln_patchify_kernel)."""
    _lnp_case(DTYPES[dt], 96, H, H, 2, "generic", shift=1)


def _pool_case(dtype, C, HW, nimg, **rows_kw):
    """gcv_k_pool_ln, or gcv_k_pool_ln_rows with the row mapping of `rows_kw`, against kcases.pool_ln.  The output buffer is
    sentinel-filled and two rows longer than the last mapped row: only the mapped rows may be written."""
    case = kcases.pool_ln(C, HW, nimg, dtype, **rows_kw)
    i = case.inputs
    nrows = max(case.rows) + 3
    out = torch.full((nrows, C), SENT, dtype=dtype, device=dev())
    args = (_lib.dtype_code(dtype), ptr(D(i["x"], dtype)), ptr(D(i["lw"])), ptr(D(i["lb"])), ptr(out), nimg, HW, C, 1e-6)
    if rows_kw:
        kutil.call("gcv_k_pool_ln_rows", *args, rows_kw["seg_n"], rows_kw["row_stride"], rows_kw["row0"])
    else:
        kutil.call("gcv_k_pool_ln", *args)
    others = [r for r in range(nrows) if r not in case.rows]
    assert (out[others].float() == SENT).all(), f"a row outside {case.rows} was written"
    case.assert_close(out[case.rows])


@pytest.mark.parametrize("dt", ALL)
@pytest.mark.parametrize("HW", [49, 9])
def test_avgpool_layernorm(dt, HW):
    _pool_case(DTYPES[dt], 768, HW, 5)


@pytest.mark.parametrize("dt", ALL)
@pytest.mark.parametrize("C,HW,nimg", [(768, 1, 3), (1536, 9, 2), (1536, 49, 4)])
def test_avgpool_layernorm_single_token_and_wide(dt, C, HW, nimg):
    """a single token (res 32), and pool_ln_kernel<T, 6> (ConvNeXt-L, C = 1536)"""
    _pool_case(DTYPES[dt], C, HW, nimg)


@pytest.mark.parametrize("dt", ALL)
@pytest.mark.parametrize("C", [768, 1536])
@pytest.mark.parametrize("nimg,seg_n,row_stride,row0", [(6, 3, 2, 0),       # rows 0, 2, 4, 1, 3, 5
                                                        (3, 3, 2, 1)])      # rows 1, 3, 5; rows 0, 2, 4 keep the sentinel
def test_avgpool_layernorm_row_mapping(dt, C, nimg, seg_n, row_stride, row0):
    """The mapping the networks use to interleave their passes' rows (csrc/net_impl.h): image b -> row
    (b % seg_n) * row_stride + row0 + b / seg_n, through gcv_k_pool_ln_rows."""
    _pool_case(DTYPES[dt], C, 9, nimg, seg_n=seg_n, row_stride=row_stride, row0=row0)




def _ln_rows_case(dtype, rows, C):
    """gcv_k_layernorm_rows against kcases.layernorm_rows, the result in the middle of a sentinel-filled buffer: two rows of
    guard in front and behind.  Where C is no multiple of 64 the buffer is laid out with 64 ceil(C / 64) columns per row; the
    kernel writes dense rows, so all it may touch is the first rows x C elements behind the front guard."""
    case = kcases.layernorm_rows(rows, C, dtype)
    i = case.inputs
    Cp = 64 * -(-C // 64)
    buf = torch.full(((rows + 4) * Cp,), SENT, dtype=dtype, device=dev())
    out = buf[2 * Cp:2 * Cp + rows * C]
    kutil.call("gcv_k_layernorm_rows", _lib.dtype_code(dtype), ptr(D(i["x"], dtype)), ptr(D(i["lw"])), ptr(D(i["lb"])),
               ptr(out), rows, C, 1e-5)
    assert (buf[:2 * Cp].float() == SENT).all(), "written in front of the first row"
    assert (buf[2 * Cp + rows * C:].float() == SENT).all(), "written behind the last row"
    case.assert_close(out.reshape(rows, C))


@pytest.mark.parametrize("dt", ALL)
@pytest.mark.parametrize("C", [96, 384, 1536])
def test_layernorm_rows(dt, C):
    _ln_rows_case(DTYPES[dt], 37, C)


@pytest.mark.parametrize("dt", ALL)
@pytest.mark.parametrize("rows,C", [(1, 768),       # one row: one live wave of the workgroup
                                    (5, 96),        # a second workgroup with one live wave; half of the second register's lanes
                                    (4, 100),       # C no multiple of 64: the c < C guards of a partly filled register
                                    (3, 1536)])     # all 24 registers
def test_layernorm_rows_one_row_ragged_width_and_full_width(dt, rows, C):
    _ln_rows_case(DTYPES[dt], rows, C)


# ----------------------------------------------------------------------------- AE / VAE small kernels
def _conv3_takes_matrix_pipe(dtype, x_ptr, out_ptr, bias_ptr, sb, sc, sy, sx, H, W):
    """launch_conv3_first's own test (csrc/kernels_impl.h): conv3_first_mfma_kernel for 16-bit storage, unit column stride,
    W a multiple of 32 up to 224, H a multiple of 8, strides that are multiples of 8, x and bias 16-byte and `out` 8-byte
    aligned; else conv3_first_kernel"""
    return (dtype != torch.float32 and sx == 1 and W % 32 == 0 and W <= 224 and H % 8 == 0 and (sb | sc | sy) % 8 == 0
            and x_ptr % 16 == 0 and out_ptr % 8 == 0 and bias_ptr % 16 == 0)


def _conv3_case(dtype, n, H, W, pool, kernel, pad=0, strides="nchw"):
    """gcv_k_conv3_first against kcases.conv3_first.  `pad`: NCHW frames cut out of a buffer whose rows are `pad` elements
    longer (filled with 3); strides "nhwc": the frame uploaded channels-last (sc = 1, sx = 3).  `kernel` ("mfma" / "valu") is
    asserted by the launcher's own rule.  Eight pixels of sentinel behind the output."""
    case = kcases.conv3_first(n, H, W, pool, dtype, strides)
    i = case.inputs
    if strides == "nchw":
        frame = torch.full((n, 3, H, W + pad), 3.0)
        frame[..., :W] = i["x"]
        st = (3 * H * (W + pad), H * (W + pad), W + pad, 1)
    else:
        assert pad == 0
        frame, st = i["x"].permute(0, 2, 3, 1).contiguous(), (H * W * 3, 1, W * 3, 3)
    xd, bias = D(frame, dtype), D(i["bias"])
    P = n * (H // 2) * (W // 2)
    out = torch.full((P + 8, 16), SENT, dtype=dtype, device=dev())
    takes = _conv3_takes_matrix_pipe(dtype, xd.data_ptr(), out.data_ptr(), bias.data_ptr(), *st, H, W)
    assert takes == (kernel == "mfma"), f"this launch does not reach the {kernel} kernel"
    wp = D(i["w"].permute(2, 3, 1, 0).reshape(27, 16).contiguous())
    kutil.call("gcv_k_conv3_first", _lib.dtype_code(dtype), ptr(xd), *st, ptr(wp), ptr(bias), ptr(out), n, H, W, int(pool),
               1 if pool else 3)
    assert (out[P:].float() == SENT).all(), "written behind the last pixel"
    case.assert_close(out[:P].reshape(n, H // 2, W // 2, 16))


@pytest.mark.parametrize("dt", ALL)
@pytest.mark.parametrize("pool", [True, False])
@pytest.mark.parametrize("H", [32, 224, 20])          # 20: not a multiple of 8 -> the VALU kernel for every dtype
def test_first_conv_3_to_16(dt, pool, H):
    dtype = DTYPES[dt]
    _conv3_case(dtype, 2, H, H, pool, "valu" if (dtype == torch.float32 or H == 20) else "mfma")


@pytest.mark.parametrize("dt", H16)
@pytest.mark.parametrize("pool", [True, False])
@pytest.mark.parametrize("n,H,W,pad", [(1, 8, 32, 0),         # one band, one column group
                                       (3, 16, 96, 0),        # three column groups (it / ncg with ncg no power of two), two bands
                                       (2, 24, 64, 0),        # a middle band: no zero rows above or below
                                       (1, 8, 224, 0),        # the widest frame the LDS band holds
                                       (2, 16, 32, 8)])       # row stride W + 8
def test_first_conv_matrix_pipe_kernel(dt, pool, n, H, W, pad):
    """conv3_first_mfma_kernel<T, POOL> off the square frames: non-square, several column groups and bands, a row stride
    that is not the width"""
    _conv3_case(DTYPES[dt], n, H, W, pool, "mfma", pad=pad)


@pytest.mark.parametrize("dt", ALL)
@pytest.mark.parametrize("pool", [True, False])
@pytest.mark.parametrize("n,H,W", [(2, 20, 28),      # 280 pooled pixels: two blocks, the second mostly dead lanes
                                   (1, 34, 18)])
def test_first_conv_valu_kernel(dt, pool, n, H, W):
    _conv3_case(DTYPES[dt], n, H, W, pool, "valu")


@pytest.mark.parametrize("dt", H16)
@pytest.mark.parametrize("pool", [True, False])
def test_first_conv_valu_kernel_16bit_width_no_multiple_of_32(dt, pool):
    """W = 48: W % 32 != 0 keeps an otherwise eligible 16-bit launch off the matrix pipe"""
    _conv3_case(DTYPES[dt], 2, 8, 48, pool, "valu")


@pytest.mark.parametrize("pool", [True, False])
def test_first_conv_valu_kernel_fp32_channels_last_frame(pool):
    """the frame addressed with NHWC strides (sc = 1, sx = 3)"""
    _conv3_case(torch.float32, 2, 20, 28, pool, "valu", strides="nhwc")


def _convt2_case(dtype, n, H, W, act):
    """gcv_k_convt2_small against kcases.convt2_small; eight pixels of sentinel behind the output"""
    case = kcases.convt2_small(n, H, W, act, dtype)
    i = case.inputs
    P = n * 2 * H * 2 * W
    out = torch.full((P + 8, 3), SENT, dtype=dtype, device=dev())
    kutil.call("gcv_k_convt2_small", _lib.dtype_code(dtype), ptr(D(i["x"].permute(0, 2, 3, 1).contiguous(), dtype)),
               ptr(D(i["w"].permute(0, 2, 3, 1).reshape(16, 12).contiguous())), ptr(D(i["bias"])), ptr(out), n, H, W, act)
    assert (out[P:].float() == SENT).all(), "written behind the last pixel"
    case.assert_close(out[:P].reshape(n, 2 * H, 2 * W, 3))


@pytest.mark.parametrize("dt", ALL)
@pytest.mark.parametrize("act", [1, 3])
def test_last_conv_transpose_16_to_3(dt, act):
    _convt2_case(DTYPES[dt], 2, 12, 12, act)


@pytest.mark.parametrize("dt", ALL)
@pytest.mark.parametrize("act", [1, 3])
@pytest.mark.parametrize("n,H,W", [(1, 1, 1), (3, 5, 7), (1, 3, 90)])
def test_last_conv_transpose_16_to_3_one_pixel_and_odd_maps(dt, act, n, H, W):
    """one pixel; odd non-square maps of 105 and 270 pixels: a ragged block, and a second one"""
    _convt2_case(DTYPES[dt], n, H, W, act)


def _reparam_case(dtype, B, S, with_mu=True):
    case = kcases.reparam(B, S, dtype)
    i = case.inputs
    N = kcases.REPARAM_N
    mu_out = torch.full((B + 1, N), SENT, dtype=torch.float32, device=dev()) if with_mu else None
    zout = torch.full((B + 1, N), SENT, dtype=dtype, device=dev())
    kutil.call("gcv_k_reparam", _lib.dtype_code(dtype), ptr(D(i["part"])), S, ptr(D(i["bias"])), ptr(D(i["eps"])),
               ptr(mu_out), ptr(zout), B, N)
    assert (zout[B].float() == SENT).all() and (mu_out is None or (mu_out[B] == SENT).all()), "written behind row B"
    case.assert_close({"z": zout[:B], **({"mu": mu_out[:B]} if with_mu else {})})


@pytest.mark.parametrize("dt", ALL)
def test_reparameterise_from_splitk(dt):
    """z = eps*exp(0.5*mu) + mu with std taken from mu (model/genconvit_vae.py:45-47), written NHWC."""
    _reparam_case(DTYPES[dt], 3, 4)


@pytest.mark.parametrize("dt", ALL)
def test_reparameterise_one_row_one_slab(dt):
    _reparam_case(DTYPES[dt], 1, 1)


@pytest.mark.parametrize("dt", ALL)
def test_reparameterise_without_mu_output(dt):
    """mu_out = NULL: z alone"""
    _reparam_case(DTYPES[dt], 3, 4, with_mu=False)


def _head_tail_case(dtype, B, K):
    case = kcases.head_tail(B, K, dtype)
    i = case.inputs
    out = torch.full((B + 1, 2), SENT, dtype=torch.float32, device=dev())
    kutil.call("gcv_k_head_tail", _lib.dtype_code(dtype), ptr(D(i["h"], dtype)), ptr(D(i["w"])), ptr(D(i["b"])),
               ptr(out), B, K)
    assert (out[B] == SENT).all(), "written behind row B"
    case.assert_close(out[:B])


@pytest.mark.parametrize("dt", ALL)
def test_head_tail(dt):
    _head_tail_case(DTYPES[dt], 9, 500)       # 9 rows: a third workgroup with one live wave


@pytest.mark.parametrize("dt", ALL)
@pytest.mark.parametrize("B,K", [(1, 500), (6, 64)])       # K = 64: one trip of the lane-stride loop
def test_head_tail_one_row_and_one_trip(dt, B, K):
    _head_tail_case(DTYPES[dt], B, K)


def _head_splitk_case(dtype, B, K, S, act):
    """The head as the networks run it: fc's split-K partials summed, + bias, ReLU (vae) / exact GELU (ed), rounded to the
    storage dtype, then fc2 (model/genconvit_ed.py:87, model/genconvit_vae.py:114).  In 16-bit storage the bound of a row
    allows for its hidden units next to a rounding tie (kcases.head_tail_splitk)."""
    case = kcases.head_tail_splitk(B, K, S, act, dtype)
    i = case.inputs
    out = torch.full((B + 1, 2), SENT, dtype=torch.float32, device=dev())
    kutil.call("gcv_k_head_tail_splitk", _lib.dtype_code(dtype), ptr(D(i["part"])), S, ptr(D(i["b1"])), act, ptr(D(i["w"])),
               ptr(D(i["b"])), ptr(out), B, K)
    assert (out[B] == SENT).all(), "written behind row B"
    case.assert_close(out[:B])


@pytest.mark.parametrize("dt", ALL)
@pytest.mark.parametrize("act", [1, 2])
def test_head_tail_with_splitk_reduce(dt, act):
    _head_splitk_case(DTYPES[dt], 37, 500, 8, act)


@pytest.mark.parametrize("dt", ALL)
@pytest.mark.parametrize("act", [1, 2])
@pytest.mark.parametrize("B,K,S", [(1, 500, 1), (5, 300, 3)])
def test_head_tail_with_splitk_reduce_one_slab_and_short_rows(dt, act, B, K, S):
    """one row of one slab; K = 300: the second trip of the thread-stride loop has 44 live threads"""
    _head_splitk_case(DTYPES[dt], B, K, S, act)


@pytest.mark.parametrize("dt", ALL)
def test_bilinear_resize_and_mse(dt):
    """transforms.Resize((224,224)) of x_hat (genconvit_vae.py:116) + per-frame MSE (train/train_vae.py:24): the three ways
    the launcher is called.  Both outputs, msepart compared block by block; no recon; no mse, where msepart must stay
    untouched."""
    dtype = DTYPES[dt]
    B = 2
    case = kcases.resize_mse(B, dtype)
    xhat, img = D(case.inputs["xhat"].permute(0, 2, 3, 1).contiguous(), dtype), D(case.inputs["img"], dtype)

    def launch(with_recon, with_mse):
        recon = torch.full((B + 1, 3, 224, 224), SENT, dtype=dtype, device=dev()) if with_recon else None
        msepart = torch.full((B + 1, 196), SENT, dtype=torch.float32, device=dev())
        mse = torch.full((B + 1,), SENT, dtype=torch.float32, device=dev()) if with_mse else None
        kutil.call("gcv_k_resize_mse", _lib.dtype_code(dtype), ptr(xhat), ptr(img), ptr(recon), ptr(msepart), ptr(mse), B)
        assert recon is None or (recon[B].float() == SENT).all(), "recon written behind frame B"
        assert (msepart[B] == SENT).all() and (mse is None or mse[B] == SENT), "msepart / mse written behind frame B"
        return recon, msepart, mse

    recon, msepart, mse = launch(True, True)
    case.assert_close({"recon": recon[:B], "msepart": msepart[:B], "mse": mse[:B]})
    _, msepart, mse = launch(False, True)
    case.assert_close({"msepart": msepart[:B], "mse": mse[:B]})
    recon, msepart, _ = launch(True, False)
    assert (msepart == SENT).all(), "msepart written by a launch without mse"
    case.assert_close({"recon": recon[:B]})




def test_vote_sigmoid_mean():
    logits = rnd((37, 2), 1, 3.0)
    got = _lib.vote(logits.to(dev()))
    torch.cuda.synchronize()
    assert_close(got, torch.sigmoid(logits).mean(0), 1e-6, "vote")


@pytest.mark.parametrize("rows", [1, 256, 257, 1000])
def test_vote_sigmoid_mean_across_waves_and_loop_trips(rows):
    """vote_kernel is one 256-thread block: the 37 rows above are one wave and one trip of its stride loop.  256 rows fill
    all four waves once, 257 and 1000 take further trips, so the cross-wave sum and the loop carry weight; 1 row is the
    mean's degenerate case.  Logits span +-30 (fp32 sigmoid is 0 or 1 beyond about +-17) in seeded random order; against
    float64."""
    logits = torch.linspace(-30.0, 30.0, 2 * rows)[torch.randperm(2 * rows, generator=torch.Generator().manual_seed(1))]
    logits = logits.reshape(rows, 2).contiguous()
    got = _lib.vote(logits.to(dev()))
    torch.cuda.synchronize()
    want = torch.sigmoid(logits.double()).mean(0)
    err = (got.double().cpu() - want).abs().max().item()
    assert err <= 1e-6, f"vote over {rows} rows: max abs err {err:.3e} > 1e-6"


# ----------------------------------------------------------------------------- error behaviour
def test_errors_are_raised_not_swallowed():
    with pytest.raises(_lib.GenConViTHipError, match="multiple of the 16-byte chunk"):
        A = torch.zeros((4, 6), device=dev())
        gemm(torch.float32, _lib.A_PLAIN, _lib.EPI_BIAS_ACT, A, A, A, 4, 4, 6, lda=6, ldc=4)
    with pytest.raises(_lib.GenConViTHipError, match="C must be one of"):
        x = torch.zeros((1, 7, 7, 100), device=dev())
        kutil.call("gcv_k_dwconv7_ln", 0, ptr(x), ptr(x), ptr(x), ptr(x), ptr(x), ptr(x), 1, 7, 7, 100, 1e-6)


# ----------------------------------------------------------------------------- Swin-T pieces (row A6)
def swin_attn_case(dtype, B, H, W, C, nH, shift, kernel, qkv_off=0, out_off=0, variant="benign"):
    """gcv_k_swin_window_attn against kcases.swin_attn.  The result lies in the middle of a sentinel-filled buffer, one row
    of W tokens of guard in front and behind; the whole buffer is sentinel before the launch, so a token that is never
    written shows too.  `qkv_off` / `out_off`: the tensor starts that many elements into its allocation.  `kernel` ("mfma" /
    "valu") is asserted by launch_swin_window_attn's own rule (csrc/kernels_impl.h): swin_window_attn_mfma_kernel for 16-bit
    storage when `(qkv & 15) == 0 && (out & 7) == 0 && C % 8 == 0`, else swin_window_attn_kernel<T>.  Also used by
    tests/test_numerics_gpu.py."""
    case = kcases.swin_attn(B, H, W, C, nH, shift, dtype, variant=variant)
    i = case.inputs
    n_in, n_out, guard = B * H * W * 3 * C, B * H * W * C, W * C
    qbuf = torch.zeros((n_in + 8,), dtype=dtype, device=dev())
    qkv = qbuf[qkv_off:qkv_off + n_in]
    qkv.copy_(i["qkv"].reshape(-1).to(dev(), dtype))
    obuf = torch.full((n_out + 2 * guard + 8,), SENT, dtype=dtype, device=dev())
    out = obuf[guard + out_off:guard + out_off + n_out]
    mfma = dtype != torch.float32 and qkv.data_ptr() % 16 == 0 and out.data_ptr() % 8 == 0 and C % 8 == 0
    assert mfma == (kernel == "mfma"), f"this launch does not reach the {kernel} kernel"
    kutil.call("gcv_k_swin_window_attn", _lib.dtype_code(dtype), ptr(qkv), ptr(D(i["table"])), ptr(out), B, H, W, C, nH, shift)
    assert (obuf[:guard + out_off].float() == SENT).all(), "written in front of the first token"
    assert (obuf[guard + out_off + n_out:].float() == SENT).all(), "written behind the last token"
    got = out.reshape(B, H, W, C)
    assert torch.isfinite(got.float()).all(), "non-finite attention output"
    case.assert_close(got)
    return case


def _attn_kernel(dtype):
    return "valu" if dtype == torch.float32 else "mfma"


@pytest.mark.parametrize("dt", ALL)
@pytest.mark.parametrize("H,C,nH,shift", [(14, 96, 3, 0), (14, 96, 3, 3), (28, 192, 6, 3), (7, 768, 24, 0)])
def test_swin_window_attention(dt, H, C, nH, shift):
    """W-MSA / SW-MSA (timm 0.6.5 WindowAttention + cyclic shift + mask) on a (B,H,W,3C) qkv tensor: the network's square maps"""
    dtype = DTYPES[dt]
    swin_attn_case(dtype, 2, H, H, C, nH, shift, _attn_kernel(dtype))


@pytest.mark.parametrize("dt", ALL)
@pytest.mark.parametrize("B,H,W,C,nH,shift", [
    (1, 7, 7, 32, 1, 0),        # one window, one head
    (2, 14, 21, 96, 3, 3),      # off-square, nWy != nWx, all nine mask regions
    (2, 21, 14, 96, 3, 0),      # the other orientation, unshifted
    (2, 14, 7, 64, 2, 3),       # shift 3 at W = 7 (the launcher only requires H > 7): x region 0 is empty
    (1, 7, 7, 768, 24, 0),      # the table's head stride at the largest nH
])
def test_swin_window_attention_off_square_maps(dt, B, H, W, C, nH, shift):
    """fp32 storage on swin_window_attn_kernel, 16-bit on swin_window_attn_mfma_kernel"""
    dtype = DTYPES[dt]
    swin_attn_case(dtype, B, H, W, C, nH, shift, _attn_kernel(dtype))


@pytest.mark.parametrize("dt", H16)
@pytest.mark.parametrize("qkv_off,out_off", [(1, 0),       # qkv 2-byte aligned: (qkv & 15) != 0
                                             (0, 2)])      # out 4 bytes into its allocation: (out & 7) != 0
def test_swin_window_attention_valu_kernel_in_16bit_storage(dt, qkv_off, out_off):
    """swin_window_attn_kernel<half_t> / <bf16_t>: the launcher takes it for 16-bit storage only when
    `(qkv & 15) == 0 && (out & 7) == 0 && C % 8 == 0` fails, which a fresh allocation never does"""
    swin_attn_case(DTYPES[dt], 2, 14, 21, 96, 3, 3, "valu", qkv_off=qkv_off, out_off=out_off)


def _patch_merge_case(dtype, C, H, W, n):
    """gcv_k_patch_merge_ln against kcases.patch_merge_ln; two rows of sentinel in front of and behind the result"""
    case = kcases.patch_merge_ln(C, H, W, n, dtype)
    i = case.inputs
    rows = n * (H // 2) * (W // 2)
    buf = torch.full((rows + 4, 4 * C), SENT, dtype=dtype, device=dev())
    kutil.call("gcv_k_patch_merge_ln", _lib.dtype_code(dtype), ptr(D(i["x"], dtype)), ptr(D(i["lw"])), ptr(D(i["lb"])),
               ptr(buf[2:]), n, H, W, C, 1e-5)
    assert (buf[:2].float() == SENT).all() and (buf[rows + 2:].float() == SENT).all(), "written outside the merged rows"
    case.assert_close(buf[2:rows + 2].reshape(n, H // 2, W // 2, 4 * C))


@pytest.mark.parametrize("dt", ALL)
@pytest.mark.parametrize("C,H", [(96, 56), (192, 28), (384, 14)])
def test_swin_patch_merging_layernorm(dt, C, H):
    _patch_merge_case(DTYPES[dt], C, H, H, 2)


@pytest.mark.parametrize("dt", ALL)
@pytest.mark.parametrize("C,H,W,n", [(96, 2, 2, 1),        # one row
                                     (96, 6, 10, 3),       # off-square; 45 rows: the last workgroup has one live wave
                                     (384, 4, 2, 2)])      # 4C = 1536: all 24 registers
def test_swin_patch_merging_layernorm_one_row_off_square_and_widest(dt, C, H, W, n):
    _patch_merge_case(DTYPES[dt], C, H, W, n)


def _mean_tokens_case(dtype, n, L, C):
    """gcv_k_mean_tokens against kcases.mean_tokens.  The buffer has 256 ceil(C / 256) columns per image and two images of
    guard in front and behind; the kernel writes dense rows: the first n x C elements behind the front guard"""
    case = kcases.mean_tokens(n, L, C, dtype)
    Cp = 256 * -(-C // 256)
    buf = torch.full(((n + 4) * Cp,), SENT, dtype=dtype, device=dev())
    out = buf[2 * Cp:2 * Cp + n * C]
    kutil.call("gcv_k_mean_tokens", _lib.dtype_code(dtype), ptr(D(case.inputs["x"], dtype)), ptr(out), n, L, C)
    assert (buf[:2 * Cp].float() == SENT).all(), "written in front of the first image"
    assert (buf[2 * Cp + n * C:].float() == SENT).all(), "written behind the last image"
    case.assert_close(out.reshape(n, C))


@pytest.mark.parametrize("dt", ALL)
def test_mean_over_tokens(dt):
    _mean_tokens_case(DTYPES[dt], 3, 49, 768)


@pytest.mark.parametrize("dt", ALL)
@pytest.mark.parametrize("n,L,C", [(2, 1, 96),        # one token; less than one trip of the 256-stride loop
                                   (3, 5, 300)])      # a second trip with 44 live threads
def test_mean_over_tokens_one_token_and_ragged_width(dt, n, L, C):
    _mean_tokens_case(DTYPES[dt], n, L, C)


# ----------------------------------------------------------------------------- fused ConvNeXt MLP
@pytest.mark.parametrize("dt", ["bf16", "f16"])
@pytest.mark.parametrize("C,M", [(96, 256), (96, 1000), (192, 300), (192, 37),
                                 (96, 70013),       # >= 65536 tokens at C=96: the LDS-resident persistent kernel
                                 (192, 70013),      # C=192 x-stationary kernel: 274 passes on 256 workgroups, i.e. a second pass (ring wrap-around, x reload) in some
                                 # C=384 kernel pair (kcases.PAIR384_M): 128, 1000, 6272 are small launches, 128-token pw2 tiles,
                                 # pw1 hidden range split up to 24 ways; 40000 is 157 tiles (hidden range split, 256x192 pw2
                                 # tiles); 60013 is 235 token tiles: unsplit pw1, full-width 256x384 pw2 tiles, ragged last block
                                 ] + [(384, M) for M in kcases.PAIR384_M])
def test_fused_mlp_layerscale_residual(dt, C, M):
    """timm ConvNeXtBlock tail: fc1 -> exact GELU -> fc2 -> * gamma -> + shortcut, hidden kept on chip."""
    mlp_case(DTYPES[dt], C, M)


@pytest.mark.parametrize("dt", ["bf16", "f16"])
@pytest.mark.parametrize("M", kcases.PAIR384_SPLIT_M + kcases.PAIR384_TILE_M)
def test_fused_mlp_c384_at_every_hidden_range_split(dt, M):
    """The C = 384 pw1 kernel at the splits the cases above leave out, ns = 12, 6, 4, 2: 4, 8, 12 and 24 hidden chunks per
    workgroup on a ring of depth 6 (shorter than the ring, the first wrap, two and four wraps), each at the smallest token
    count with that split, whose last 256-token tile holds one token.  The networks run them from ED at B = 8 on.  Then
    ns = 4, 3 and 2 beside the pw2 tiles the networks also pair them with (kcases.PAIR384_TILE_M)."""
    mlp_case(DTYPES[dt], 384, M)


@pytest.mark.parametrize("dt", ["bf16", "f16"])
@pytest.mark.parametrize("C,shape,wg_cap", kcases.PERSISTENT)
def test_fused_mlp_persistent_kernels_at_every_pass_count(dt, C, shape, wg_cap):
    """xs_mlp_kernel and fused_mlp_res_kernel, plain and with the LN-patchify epilogue, at one, two and four or five passes per
    workgroup (tiles per wave): a workgroup cap below the networks' 256 gives a few thousand tokens the middle passes, with
    a predecessor and a successor, that a batch of 128 runs (kcases.PERSISTENT, held against the census by
    tests/test_host_cpu.py)."""
    if isinstance(shape, list):
        mlp_lnp_case(DTYPES[dt], C, shape, wg_cap=wg_cap)
    else:
        mlp_case(DTYPES[dt], C, shape, wg_cap=wg_cap)


def mlp_case(dtype, C, M, wg_cap=0, **kw):
    """gcv_k_fused_mlp in place on the shortcut, against kcases.fused_mlp; the rows behind M carry a sentinel.  Also used
    by tests/test_mlp_bias_init_gpu.py.  wg_cap > 0: gcv_k_fused_mlp_planned, the persistent kernels on at most wg_cap
    workgroups."""
    case = kcases.fused_mlp(C, M, dtype, **kw)
    i = case.inputs
    out = torch.full((M + 8, C), 7.0, dtype=dtype, device=dev())
    out[:M] = i["res"].to(dev(), dtype)
    planned = ("gcv_k_fused_mlp_planned", (wg_cap,)) if wg_cap > 0 else ("gcv_k_fused_mlp", ())
    kutil.call(planned[0], _lib.dtype_code(dtype), C, ptr(D(i["x"], dtype)), ptr(D(i["w1"], dtype)), ptr(D(i["b1"])),
               ptr(D(i["w2"])), ptr(D(i["b2"])), ptr(D(i["gamma"])), ptr(out), ptr(out), M, *planned[1])
    assert (out[M:].float() == 7.0).all(), "rows past M were written"
    case.assert_close(out[:M])


@pytest.mark.parametrize("dt", ["bf16", "f16"])
@pytest.mark.parametrize("C,M", [(C, M) for C in (96, 192, 384) for M in (1, 4, 16, 64, 33, 129)])
def test_fused_mlp_at_a_handful_of_tokens(dt, C, M):
    """One frame at res 32 is 64 / 16 / 4 / 1 tokens at stages 0 - 3: the fused MLP kinds (Fused96, Xs192, Pair384) far below
    one token tile, and one token above a 32- and a 128-token tile.  The rows behind M carry a sentinel."""
    mlp_case(DTYPES[dt], C, M)


@pytest.mark.parametrize("dt", ALL)
@pytest.mark.parametrize("M", gemmcases.STAGE3_ROWS)
@pytest.mark.parametrize("N,K", gemmcases.STAGE3_NK)
@pytest.mark.parametrize("epi", list(gemmcases.STAGE3_KERNEL))
def test_gemm_at_one_and_three_rows_with_stage3_shapes(dt, M, N, K, epi):
    """The tile GEMMs of ConvNeXt-T's stage 3 (fc1, fc2, the down-sampling conv) as one small-resolution frame runs them:
    1 token at res 32, a few for a small batch.  Rows behind M carry a sentinel."""
    dtype = DTYPES[dt]
    A, W = q(rnd((M, K), 1), dtype), q(rnd((N, K), 2, 1 / math.sqrt(K)), dtype)
    bias = rnd((N,), 3, 0.1)
    C = torch.full((M + 8, N), 7.0, dtype=dtype, device=dev())
    if epi == "bias_gelu":
        gemm(dtype, _lib.A_PLAIN, _lib.EPI_BIAS_ACT, D(A, dtype), D(W, dtype), C, M, N, K, lda=K, ldc=N, bias=D(bias), act=2)
        want = F.gelu(A @ W.t() + bias)
    else:
        gamma, X = rnd((N,), 4, 0.5), q(rnd((M, N), 5), dtype)
        C[:M] = X.to(dev(), dtype)
        gemm(dtype, _lib.A_PLAIN, _lib.EPI_RESID, D(A, dtype), D(W, dtype), C, M, N, K, lda=K, ldc=N, bias=D(bias),
             gamma=D(gamma), resid=C)
        want = X + gamma * (A @ W.t() + bias)
    assert (C[M:].float() == 7.0).all(), "rows past M were written"
    assert_close(C[:M], want, tol(dtype, 2.0), f"gemm {epi} M={M}")


@pytest.mark.parametrize("dt", ALL)
def test_gemm_rejects_a_misaligned_operand(dt):
    """The GEMM kernels read A and Wt in 16-byte pieces; launch_gemm has no unaligned kernel behind them and refuses the
    launch.  Asserted as the error it is: nothing is launched, C keeps its sentinel."""
    dtype = DTYPES[dt]
    M, N, K = 8, 64, 64
    buf = torch.zeros((M * K + 1,), dtype=dtype, device=dev())
    W = torch.zeros((N, K), dtype=dtype, device=dev())
    C = torch.full((M, N), 7.0, dtype=dtype, device=dev())
    for A, Wt in ((buf[1:], W), (W, buf[1:])):
        assert A.data_ptr() % 16 or Wt.data_ptr() % 16
        with pytest.raises(_lib.GenConViTHipError, match="A/Wt must be 16-byte aligned"):
            gemm(dtype, _lib.A_PLAIN, _lib.EPI_BIAS_ACT, A, Wt, C, M, N, K, lda=K, ldc=N)
    torch.cuda.synchronize()
    assert (C.float() == 7.0).all()


# segments: (images, H, W) per segment, in token order
_LNP_CASES = [
    (96, [(22, 56, 56)]),                          # one segment, 68 992 tokens: 2 156 wave tiles, none ragged
    (96, [(21, 56, 56), (7, 28, 28)]),             # 65 856 + 5 488 tokens: the boundary is a tile edge (2 058 * 32)
    (96, [(21, 56, 56), (9, 28, 28), (3, 14, 14)]),   # three geometries, last tile ragged (73 500 tokens)
    (96, [(5, 56, 56), (67, 28, 28)]),             # 15 680 + 52 528: odd image count behind a boundary at token 490 * 32
    (96, [(3, 30, 30), (23, 56, 54)]),             # non-square maps, boundary at 2 700 = 84 * 32 + 12: a tile straddles it
    (192, [(3, 28, 28)]),                          # 2 352 tokens: ragged last pass (9.2 passes of 256)
    (192, [(5, 28, 28), (5, 14, 14)]),             # 3 920 + 980: boundary at 122 * 32 + 16, inside a wave tile
    (192, [(1, 14, 14), (2, 28, 28), (3, 6, 10)]),   # boundary at 196 = 6 * 32 + 4, non-square tail segment, 1 944 tokens
    (192, [(67, 28, 28), (67, 14, 14)]),           # 65 660 tokens: 257 passes on 256 persistent workgroups (second pass)
    (192, [(1, 2, 2)]),                            # one frame at res 32 on a ConvNeXt-T handle: 4 tokens, one patch row
    (192, [(1, 4, 4)]),                            # ... on a ConvNeXt-L handle (stage 0 is 8 x 8, C = 192; this is 16 tokens)
    (192, [(3, 2, 2), (1, 4, 4)]),                 # 12 + 16 tokens
]


@pytest.mark.parametrize("dt", ["bf16", "f16"])
@pytest.mark.parametrize("C,segs", _LNP_CASES)
def test_fused_mlp_layernorm_patchify_epilogue(dt, C, segs):
    """Last block of ConvNeXt stage 0 / 1 as the network runs it in 16-bit storage: MLP + layer scale + shortcut, then the
    stage boundary's LayerNorm2d and the 2x2 space-to-depth of its stride-2 conv in the same kernel's epilogue (timm
    ConvNeXtStage.downsample; fused_mlp_res_kernel<T, true> at C = 96, xs_mlp_kernel<T, 192, true>).  Checked element-wise
    against kcases.fused_mlp(segs=...): float64 LayerNorm of the float64 MLP output, then the patch gather, per segment."""
    mlp_lnp_case(DTYPES[dt], C, segs)


def mlp_lnp_case(dtype, C, segs, wg_cap=0, **kw):
    """gcv_k_fused_mlp_lnp on the segments (images, H, W); also used by tests/test_mlp_bias_init_gpu.py.  wg_cap > 0:
    gcv_k_fused_mlp_lnp_planned, the persistent kernels on at most wg_cap workgroups."""
    M = sum(n * h * w for n, h, w in segs)
    case = kcases.fused_mlp(C, M, dtype, segs=segs, **kw)
    i = case.inputs
    tok0, hw, wd, out0, t = [], [], [], [], 0
    for n, H, W in segs:
        tok0.append(t); hw.append(H * W); wd.append(W); out0.append(t // 4)
        t += n * H * W
    out = torch.full((M // 4 + 3, 4 * C), 7.0, dtype=dtype, device=dev())
    arr = lambda v: (ctypes.c_int * 4)(*(v + [0] * (4 - len(v))))
    a_tok0, a_hw, a_wd, a_out0 = arr(tok0), arr(hw), arr(wd), arr(out0)
    resd = D(i["res"], dtype)
    planned = ("gcv_k_fused_mlp_lnp_planned", (wg_cap,)) if wg_cap > 0 else ("gcv_k_fused_mlp_lnp", ())
    kutil.call(planned[0], _lib.dtype_code(dtype), C, ptr(D(i["x"], dtype)), ptr(D(i["w1"], dtype)),
               ptr(D(i["b1"])), ptr(D(i["w2"])), ptr(D(i["b2"])), ptr(D(i["gamma"])), ptr(resd), ptr(D(i["lw"])),
               ptr(D(i["lb"])), 1e-6, len(segs), a_tok0, a_hw, a_wd, a_out0, ptr(out), M, *planned[1])
    assert torch.equal(resd.cpu(), i["res"].to(dtype)), "the residual stream must not be written"
    assert (out[M // 4:].float() == 7.0).all(), "rows behind the last patch row were written"
    case.assert_close(out[:M // 4])


# ----------------------------------------------------------------------------- LDS-DMA pipelined GEMM
@pytest.mark.parametrize("dt", ["bf16", "f16"])
@pytest.mark.parametrize("M,N,K,act", gemmcases.cases(gemmcases.DMA_BIAS_ACT))
def test_gemm_lds_dma_pipeline_bias_act(dt, M, N, K, act):
    dtype = DTYPES[dt]
    A, W = q(rnd((M, K), 1), dtype), q(rnd((N, K), 2, 1 / math.sqrt(K)), dtype)
    bias = rnd((N,), 3, 0.1)
    C = torch.full((M, N), 7.0, dtype=dtype, device=dev())
    gemm(dtype, _lib.A_PLAIN, _lib.EPI_BIAS_ACT, D(A, dtype), D(W, dtype), C, M, N, K, lda=K, ldc=N, bias=D(bias), act=act)
    assert_close(C, act_ref(A @ W.t() + bias, act), tol(dtype, 2.0), "glds gemm")


@pytest.mark.parametrize("dt", ["bf16", "f16"])
@pytest.mark.parametrize("M,N,K", gemmcases.cases(gemmcases.DMA_RESID))
def test_gemm_lds_dma_pipeline_residual(dt, M, N, K):
    _resid_case(DTYPES[dt], M, N, K)


@pytest.mark.parametrize("dt", ["bf16", "f16"])
@pytest.mark.parametrize("M,N,K,act", gemmcases.cases(gemmcases.DMA_BIAS_ACT_MANY))
def test_gemm_lds_dma_many_tiles_bias_act(dt, M, N, K, act):
    """Several waves of tiles per CU (the B=128 shapes of stages 2/3); M has a ragged last tile."""
    dtype = DTYPES[dt]
    act = {"none": _lib.ACT_NONE, "gelu": _lib.ACT_GELU}[act]
    A, W = q(rnd((M, K), 1), dtype), q(rnd((N, K), 2, 1 / math.sqrt(K)), dtype)
    bias = rnd((N,), 3, 0.1)
    C = torch.full((M + 8, N), 7.0, dtype=dtype, device=dev())
    gemm(dtype, _lib.A_PLAIN, _lib.EPI_BIAS_ACT, D(A, dtype), D(W, dtype), C, M, N, K, lda=K, ldc=N, bias=D(bias), act=act)
    assert_close(C[:M], act_ref(A @ W.t() + bias, act), tol(dtype, 2.0), "glds gemm (many tiles)")
    assert (C[M:].float() == 7.0).all(), "rows past M must not be written"


@pytest.mark.parametrize("dt", ["bf16", "f16"])
@pytest.mark.parametrize("M,N,K", gemmcases.cases(gemmcases.DMA_RESID_MANY))
def test_gemm_lds_dma_many_tiles_residual(dt, M, N, K):
    _resid_case(DTYPES[dt], M, N, K)


def test_preprocess_frame_on_device_matches_reference_semantics():
    """Row N1: uint8 NHWC -> normalised NCHW (model/pred_func.py:95-108, dataset/loader.py:63-65,77)."""
    from genconvit_amd import synth
    from genconvit_amd.model import pred_func
    from oracle import cpu_ref
    u8 = synth.make_uint8_frames(3)
    want = cpu_ref.preprocess_frame(u8.numpy())
    got = _lib.preprocess(u8.to(dev()))
    assert got.dtype == torch.float32 and got.shape == (3, 3, 224, 224)
    assert_close(got, want, 1e-6, "preprocess fp32")
    assert_close(_lib.preprocess(u8.to(dev()), torch.float16), want, 2e-3, "preprocess fp16")
    assert_close(pred_func.preprocess_frame(u8.numpy()), want, 1e-6, "preprocess_frame drop-in")
