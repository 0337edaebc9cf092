"""Do the per-kernel GPU tests notice a kernel that is subtly wrong?  Answered without a GPU, on the builders the GPU tests
use (tests/kcases.py, and tests/camcases.py for the Grad-CAM backward kernels): per family, storage dtype and the family's
smallest case per dispatch class,
  (a) the float64 reference rounded to the storage dtype passes the comparator,
  (b) an honest float32 model passes it (float32 torch matmul / conv; the 16-bit GELU through numutil.gelu_h16_ref),
  (c) every defect of the family's catalogue is rejected, with some element at least 2 x over its bound.
(c) is a condition on the inputs and the comparator: a defect that slips through is fixed by the input distributions of
tests/kcases.py, never by dropping it.  A family with several outputs (kcases.MultiCase) passes (a) and (b) on every output
and rejects a defect on any one of them.  Each case prints its table (run with -s): the model's excess, which is the floor of
kcases.E, and err / bound of every defect."""
import pytest
import torch

from tests import camcases, kcases
from tests.kutil import DTYPES

torch.set_grad_enabled(False)

ALL = ("f32", "bf16", "f16")
H16 = ("bf16", "f16")

# (id, builder, arguments, dtypes of the family's GPU test).  Which kernel a shape reaches: csrc/cnx_mlp.h, gemm_impl.h
CASES = [
    # fused MLP: fused_mlp_kernel<T, 96, 4>, xs_mlp_kernel (192), xs_pw1 + pw2f (384), fused_mlp_res_kernel (>= 65 536)
    ("mlp-96x256", kcases.fused_mlp, (96, 256), H16),
    ("mlp-192x37", kcases.fused_mlp, (192, 37), H16),
    ("mlp-384x129", kcases.fused_mlp, (384, 129), H16),
    ("mlp-96x66049-res-kernel", kcases.fused_mlp, (96, 65536 + 513), H16),
    ("mlp-bigb2-384x129", lambda C, M, dt: kcases.fused_mlp(C, M, dt, b2_range=(2.0, 4.0)), (384, 129), H16),
    # LN-patchify epilogue: one segment, two geometries, and C = 96 (only behind the >= 65 536-token kernel)
    ("lnp-192-one-row", lambda C, segs, dt: kcases.fused_mlp(C, _tokens(segs), dt, segs=segs), (192, [(1, 2, 2)]), H16),
    ("lnp-192-two-geometries", lambda C, segs, dt: kcases.fused_mlp(C, _tokens(segs), dt, segs=segs),
     (192, [(3, 2, 2), (1, 4, 4)]), H16),
    ("lnp-96-two-geometries", lambda C, segs, dt: kcases.fused_mlp(C, _tokens(segs), dt, segs=segs),
     (96, [(21, 56, 56), (2, 6, 6)]), H16),
    # EPI_RESID: tile kernel (every dtype), LDS-DMA kernel (16-bit, K a multiple of 32 from 384 tokens on)
    ("resid-300x96x384", lambda *a: kcases.gemm("resid", *a), (300, 96, 384), ALL),
    ("resid-150x256x64", lambda *a: kcases.gemm("resid", *a), (150, 256, 64), ALL),
    ("resid-lds-dma-640x192x768", lambda *a: kcases.gemm("resid", *a), (640, 192, 768), H16),
    # EPI_BIAS_ACT with each activation
    ("bias-gelu-300x384x96", lambda M, N, K, dt: kcases.gemm("bias_act", M, N, K, dt, act=2), (300, 384, 96), ALL),
    ("bias-relu-8x1000x768", lambda M, N, K, dt: kcases.gemm("bias_act", M, N, K, dt, act=1), (8, 1000, 768), ALL),
    ("bias-leaky-256x96x48", lambda M, N, K, dt: kcases.gemm("bias_act", M, N, K, dt, act=3), (256, 96, 48), ALL),
    ("bias-none-lds-dma-513x192x32", lambda M, N, K, dt: kcases.gemm("bias_act", M, N, K, dt, act=0), (513, 192, 32), H16),
    ("conv-s2-leaky-2x16", kcases.conv3x3_s2, (2, 16, 16, 32), ALL),
    ("conv-s2-leaky-3x8", kcases.conv3x3_s2, (3, 8, 32, 64), ALL),
    ("pool4-2x16", kcases.conv3x3_pool, (2, 16, 16, 32), ALL),
    ("pool4-3x8", kcases.conv3x3_pool, (3, 8, 32, 64), ALL),
    ("convt-relu-2x7", kcases.conv_transpose2x2, (2, 7, 256, 128, 1), ALL),
    ("convt-leaky-3x14", kcases.conv_transpose2x2, (3, 14, 64, 32, 3), ALL),
    ("splitk-8x256x512", lambda M, N, K, kps, dt: kcases.gemm("splitk", M, N, K, dt, k_per_split=kps), (8, 256, 512, 128), ALL),
    ("splitk-130x128x640", lambda M, N, K, kps, dt: kcases.gemm("splitk", M, N, K, dt, k_per_split=kps), (130, 128, 640, 256),
     ALL),
    # dw7x7 + LN: tile, tiny whole-map, roll, pair and matrix-pipe kernels' smallest shapes (tests/dwcases.py)
    ("dw-tile-96x5x5", kcases.dwconv7_ln, (96, 5, 5, 1), ALL),
    ("dw-tile-one-row-192x1x13", kcases.dwconv7_ln, (192, 1, 13, 3), ALL),
    ("dw-tiny-768x3x3", kcases.dwconv7_ln, (768, 3, 3, 3), ALL),
    ("dw-roll-384x2x7", kcases.dwconv7_ln, (384, 2, 7, 4), ALL),
    ("dw-pair-1536x5x7", kcases.dwconv7_ln, (1536, 5, 7, 3), ALL),
    ("dw-mfma-96x5x56x717", kcases.dwconv7_ln, (96, 5, 56, 717), H16),      # taps rounded to T, as that kernel does
    # ... and one launch of several bands per image for each band kernel (two images under the plan of a larger launch, as
    # tests/dwcases.py GEOMETRY runs them): the two band-seam defects join the catalogue
    ("dw-roll-two-7-row-bands", lambda C, H, p, dt: kcases.dwconv7_ln(C, H, H, 2, dt, plan_nimg=p), (384, 14, 65), ALL),
    ("dw-pair-2-row-bands", lambda C, H, p, dt: kcases.dwconv7_ln(C, H, H, 2, dt, plan_nimg=p), (1536, 7, 86), ALL),
    ("dw-mfma-four-14-row-bands", lambda C, H, p, dt: kcases.dwconv7_ln(C, H, H, 2, dt, plan_nimg=p), (96, 56, 64), H16),
    # stem: stem_ln_mfma_kernel (aligned 16-bit operands, both widths and layouts), stem_ln_kernel (fp32; 16-bit when
    # misaligned).  The long-stream case has the defects of 3 x 9 x 9: they do not depend on the trip count
    ("stem-mfma-96-one-token", kcases.stem, (96, 1, 1, 1, "nchw"), H16),
    ("stem-mfma-96-3x9x9", kcases.stem, (96, 3, 9, 9, "nchw"), H16),
    ("stem-mfma-192-3x9x9", kcases.stem, (192, 3, 9, 9, "nhwc"), H16),
    ("stem-valu-96-2x5x8", kcases.stem, (96, 2, 5, 8, "nchw"), ALL),
    ("stem-valu-192-3x9x9", kcases.stem, (192, 3, 9, 9, "nhwc"), ALL),
    # LN-patchify: ln_patchify_vec_kernel (C = 96 / 192 / 384 in 16-bit), ln_patchify_kernel
    ("lnp-vec-96x3x5", kcases.ln_patchify, (96, 3, 5, 1), H16),
    ("lnp-vec-192x2x2", kcases.ln_patchify, (192, 2, 2, 1), H16),
    ("lnp-vec-384x7x7", kcases.ln_patchify, (384, 7, 7, 2), H16),
    ("lnp-generic-768x5x8", kcases.ln_patchify, (768, 5, 8, 3), ALL),
    ("lnp-generic-192x9x9", kcases.ln_patchify, (192, 9, 9, 3), ALL),
    # pool + LN: pool_ln_kernel<T, 3> and <T, 6>, plain rows and the networks' row mapping
    ("pool-768x1", kcases.pool_ln, (768, 1, 3), ALL),
    ("pool-1536x9", kcases.pool_ln, (1536, 9, 2), ALL),
    ("pool-768x9", kcases.pool_ln, (768, 9, 5), ALL),
    ("pool-rows-768", lambda C, dt: kcases.pool_ln(C, 9, 6, dt, seg_n=3, row_stride=2, row0=0), (768,), ALL),
    ("pool-rows-1536", lambda C, dt: kcases.pool_ln(C, 9, 3, dt, seg_n=3, row_stride=2, row0=1), (1536,), ALL),
    # first conv: conv3_first_mfma_kernel (16-bit, W % 32 == 0, H % 8 == 0), conv3_first_kernel
    ("conv3-mfma-pool-1x8x32", kcases.conv3_first, (1, 8, 32, True), H16),
    ("conv3-mfma-s2-1x8x32", kcases.conv3_first, (1, 8, 32, False), H16),
    ("conv3-mfma-pool-3x16x96", kcases.conv3_first, (3, 16, 96, True), H16),
    ("conv3-valu-pool-1x34x18", kcases.conv3_first, (1, 34, 18, True), ALL),
    ("conv3-valu-s2-1x34x18", kcases.conv3_first, (1, 34, 18, False), ALL),
    ("conv3-valu-s2-2x8x48", kcases.conv3_first, (2, 8, 48, False), H16),
    # last convT: one kernel, a packed branch for 16-bit storage
    ("convt2-relu-1x1x1", kcases.convt2_small, (1, 1, 1, 1), ALL),
    ("convt2-leaky-1x1x1", kcases.convt2_small, (1, 1, 1, 3), ALL),
    ("convt2-relu-3x5x7", kcases.convt2_small, (3, 5, 7, 1), ALL),
    ("convt2-leaky-3x5x7", kcases.convt2_small, (3, 5, 7, 3), ALL),
    ("reparam-1x1", kcases.reparam, (1, 1), ALL),
    ("reparam-3x4", kcases.reparam, (3, 4), ALL),
    ("head-tail-1x500", kcases.head_tail, (1, 500), ALL),
    ("head-tail-6x64", kcases.head_tail, (6, 64), ALL),
    ("head-tail-9x500", kcases.head_tail, (9, 500), ALL),
    ("head-splitk-relu-1x500x1", kcases.head_tail_splitk, (1, 500, 1, 1), ALL),
    ("head-splitk-gelu-1x500x1", kcases.head_tail_splitk, (1, 500, 1, 2), ALL),
    ("head-splitk-relu-5x300x3", kcases.head_tail_splitk, (5, 300, 3, 1), ALL),
    ("head-splitk-gelu-5x300x3", kcases.head_tail_splitk, (5, 300, 3, 2), ALL),
    ("head-splitk-relu-37x500x8", kcases.head_tail_splitk, (37, 500, 8, 1), ALL),
    ("head-splitk-gelu-37x500x8", kcases.head_tail_splitk, (37, 500, 8, 2), ALL),
    ("resize-mse-2", kcases.resize_mse, (2,), ALL),
    # Swin-T (row A6): window attention (B, H, W, C, nH, shift).  16-bit storage runs swin_window_attn_mfma_kernel on aligned
    # buffers and swin_window_attn_kernel<T> on a misaligned qkv or out: same case, same comparator
    ("swin-attn-one-window", kcases.swin_attn, (1, 7, 7, 32, 1, 0), ALL),
    ("swin-attn-14x21-shifted", kcases.swin_attn, (2, 14, 21, 96, 3, 3), ALL),
    ("swin-attn-21x14", kcases.swin_attn, (2, 21, 14, 96, 3, 0), ALL),
    ("swin-attn-14x7-shifted", kcases.swin_attn, (2, 14, 7, 64, 2, 3), ALL),
    ("swin-attn-24-heads", kcases.swin_attn, (1, 7, 7, 768, 24, 0), ALL),
    ("swin-attn-28x28-shifted", kcases.swin_attn, (2, 28, 28, 192, 6, 3), ALL),
    ("patch-merge-one-row", kcases.patch_merge_ln, (96, 2, 2, 1), ALL),
    ("patch-merge-6x10", kcases.patch_merge_ln, (96, 6, 10, 3), ALL),
    ("patch-merge-384", kcases.patch_merge_ln, (384, 4, 2, 2), ALL),
    ("patch-merge-192x28x28", kcases.patch_merge_ln, (192, 28, 28, 2), ALL),
    ("mean-tokens-3x49x768", kcases.mean_tokens, (3, 49, 768), ALL),
    ("mean-tokens-one-token", kcases.mean_tokens, (2, 1, 96), ALL),
    ("mean-tokens-3x5x300", kcases.mean_tokens, (3, 5, 300), ALL),
    ("ln-rows-1x768", kcases.layernorm_rows, (1, 768), ALL),
    ("ln-rows-5x96", kcases.layernorm_rows, (5, 96), ALL),
    ("ln-rows-4x100", kcases.layernorm_rows, (4, 100), ALL),
    ("ln-rows-3x1536", kcases.layernorm_rows, (3, 1536), ALL),
    ("ln-rows-37x384", kcases.layernorm_rows, (37, 384), ALL),
    # the backward contractions' launch shape: one split of the whole K (no split edge to drop an index at)
    ("splitk-one-split-13x3072x768", lambda M, N, K, kps, dt: kcases.gemm("splitk", M, N, K, dt, k_per_split=kps),
     (13, 3072, 768, 768), ALL),
    ("splitk-one-split-13x768x3072", lambda M, N, K, kps, dt: kcases.gemm("splitk", M, N, K, dt, k_per_split=kps),
     (13, 768, 3072, 3072), ALL),
]
# the Grad-CAM backward kernels: the cases of tests/test_cam_kernels_gpu.py, every one of them (tests/camcases.py)
CASES += camcases.CASES


def _tokens(segs):
    return sum(n * h * w for n, h, w in segs)


_PARAMS = [pytest.param(build, args, dt, id=f"{name}-{dt}") for name, build, args, dts in CASES for dt in dts]


def _parts(case):
    """name -> comparator of each output (one unnamed output for a plain Case)"""
    return case.parts if isinstance(case, kcases.MultiCase) else {"": case}


def _measure(case, result, want, stored):
    """per output: the comparator's measurement of a float64 result (brought to the output buffer's dtype unless `stored`)"""
    if not isinstance(result, dict):
        result, want = {"": result}, {"": want}
    return {name: part.measure(result[name] if stored else part.to_storage(result[name]), want[name])
            for name, part in _parts(case).items()}


@pytest.mark.parametrize("build,args,dt", _PARAMS)
def test_comparator_accepts_honest_results_and_rejects_every_planted_defect(build, args, dt):
    case = build(*args, DTYPES[dt])
    want = case.want()
    for name, m in _measure(case, want, want, stored=False).items():
        assert m["ratio"] <= 1.0, f"(a) the rounded reference fails its own check: {case.what} {name}: err/bound {m['ratio']:.2f}"
    print(f"\n{case.what}:" + (f" delta {case.delta:.2e}, at most {case.near_tie} hidden units of a row next to a tie"
                               if hasattr(case, "delta") else ""))
    for name, m in _measure(case, case.model(case.inputs), want, stored=True).items():
        part = _parts(case)[name]
        print(f"  honest fp32 model {name}: excess {m['excess']:.3e}, err/bound {m['ratio']:.2f}"
              + (f" (e = {part.e:.1e})" if part.e is not None else f" (bound at most {part.tol_before:.1e})"))
        assert m["ratio"] <= 1.0, \
            f"(b) the honest float32 model fails the check: {name} err/bound {m['ratio']:.2f}, excess {m['excess']:.3e}"
    assert case.defects, "a family without a catalogue"
    missed = []
    for name, planted in case.defects.items():
        ms = _measure(case, planted(case.inputs), want, stored=False)
        ratio, err = max(m["ratio"] for m in ms.values()), max(m["err"] for m in ms.values())
        verdict = "rejected" if ratio >= 2.0 else "PASSES"
        print(f"  {name:42s} max err {err:.3e}  err/bound {ratio:9.1f}  {verdict}")
        if ratio < 2.0:
            missed.append(f"{name} (err/bound {ratio:.2f})")
    assert not missed, f"(c) {case.what}: not rejected by a factor 2: " + ", ".join(missed)


@pytest.mark.parametrize("name", [name for name, *_ in camcases.CASES])
def test_cam_closed_forms_equal_the_autograd_reference(name):
    """The float32 models and the defects of tests/camcases.py are closed forms; the reference is autograd.  Run in float64 the
    closed form equals the reference to 1e-12 of each output's largest magnitude (gaps hold the sentinel in both)."""
    case = camcases.build(name, torch.float32)
    got, want = case.closed64(), case.want()
    assert set(got) == set(want)
    for out, w in want.items():
        rel = ((got[out].double() - w).abs().max() / w.abs().max().clamp(min=1e-300)).item()
        print(f"{case.what} {out}: closed form against autograd {rel:.2e}")
        assert rel <= 1e-12, f"{case.what} {out}: {rel:.2e}"


def test_swin_reference_is_the_oracles_on_a_square_map():
    """kcases.swin_attn is written for any H x W; on a square map its index, its mask and its result are those of
    oracle/cpu_ref.py's restatement of timm (the formula the GPU test used before)"""
    from oracle.cpu_ref import _swin_attn_mask, _swin_rel_index
    assert torch.equal(kcases.swin_rel_index(), _swin_rel_index(7))
    B, H, C, nH, shift, N = 2, 14, 96, 3, 3, 49
    assert torch.equal(kcases.swin_attn_mask(H, H, shift).float(), _swin_attn_mask(H, H, 7, shift))
    case = kcases.swin_attn(B, H, H, C, nH, shift, torch.float32)
    qkv, table = case.inputs["qkv"].double(), case.inputs["table"].double()
    y = torch.roll(qkv, shifts=(-shift, -shift), dims=(1, 2))
    yw = y.view(B, H // 7, 7, H // 7, 7, 3 * C).permute(0, 1, 3, 2, 4, 5).reshape(-1, N, 3, nH, C // nH)
    qq, kk, vv = yw.permute(2, 0, 3, 1, 4).unbind(0)
    attn = (qq * (C // nH) ** -0.5) @ kk.transpose(-2, -1)
    attn = attn + table[_swin_rel_index(7).view(-1)].view(N, N, nH).permute(2, 0, 1).unsqueeze(0)
    m = _swin_attn_mask(H, H, 7, shift).double()
    attn = (attn.view(B, m.shape[0], nH, N, N) + m.unsqueeze(1).unsqueeze(0)).view(-1, nH, N, N)
    o = (attn.softmax(-1) @ vv).transpose(1, 2).reshape(-1, N, C)
    o = o.view(B, H // 7, H // 7, 7, 7, C).permute(0, 1, 3, 2, 4, 5).reshape(B, H, H, C)
    o = torch.roll(o, shifts=(shift, shift), dims=(1, 2))
    assert (case.want() - o).abs().max().item() <= 1e-14
