"""Do the per-kernel GPU tests notice a kernel that is subtly wrong?  Answered without a GPU, on the builders the GPU tests
use (tests/kcases.py): per family, storage dtype and the family's smallest case per dispatch class,
  (a) the float64 reference rounded to the storage dtype passes the comparator,
  (b) an honest float32 model passes it (float32 torch matmul / conv; the 16-bit GELU through numutil.gelu_h16_ref),
  (c) every defect of the family's catalogue is rejected, with some element at least 2 x over its bound.
(c) is a condition on the inputs and the comparator: a defect that slips through is fixed by the input distributions of
tests/kcases.py, never by dropping it.  Each case prints its table (run with -s): the model's excess, which is the floor of
kcases.E, and err / bound of every defect."""
import pytest
import torch

from tests import kcases
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
]


def _tokens(segs):
    return sum(n * h * w for n, h, w in segs)


_PARAMS = [pytest.param(build, args, dt, id=f"{name}-{dt}") for name, build, args, dts in CASES for dt in dts]


@pytest.mark.parametrize("build,args,dt", _PARAMS)
def test_comparator_accepts_honest_results_and_rejects_every_planted_defect(build, args, dt):
    case = build(*args, DTYPES[dt])
    want = case.want()
    ok, msg = case.check(case.to_storage(want), want, case.inputs)
    assert ok, f"(a) the rounded reference fails its own check: {msg}"
    m = case.measure(case.model(case.inputs), want)
    print(f"\n{case.what}: honest fp32 model: excess {m['excess']:.3e}, err/bound {m['ratio']:.2f}"
          + (f" (e = {case.e:.1e})" if case.e is not None else f" (flat bound {case.tol_before:.1e})"))
    assert m["ratio"] <= 1.0, f"(b) the honest float32 model fails the check: err/bound {m['ratio']:.2f}, excess {m['excess']:.3e}"
    assert case.defects, "a family without a catalogue"
    missed = []
    for name, planted in case.defects.items():
        d = case.measure(case.to_storage(planted(case.inputs)), want)
        verdict = "rejected" if d["ratio"] >= 2.0 else "PASSES"
        print(f"  {name:42s} max err {d['err']:.3e}  err/bound {d['ratio']:9.1f}  {verdict}")
        if d["ratio"] < 2.0:
            missed.append(f"{name} (err/bound {d['ratio']:.2f})")
    assert not missed, f"(c) {case.what}: not rejected by a factor 2: " + ", ".join(missed)
