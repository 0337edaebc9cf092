"""The launches of the GEMM family (gcv_k_gemm: tile GEMM, LDS-DMA GEMM, direct 3x3 conv) that the tests run, in one place: the
shape lists of the GPU parity tests, each case with the kernel it is meant to reach, and the launches of the networks by
formula.  tests/test_host_cpu.py asks gcv_gemm_plan, without a GPU, which kernel each of them runs: every kernel gemm_select
(csrc/gemm_impl.h) names must be the plan of at least one GPU case here, and every plan is pinned by tests/golden/gemm_plan.json."""
from collections import namedtuple

from genconvit_amd._lib import (A_IM2COL3_POOL, A_IM2COL3_S2, A_PLAIN, ACT_GELU, ACT_LEAKY, ACT_NONE, ACT_RELU, EPI_BIAS_ACT,
                                EPI_CONVT, EPI_POOL4, EPI_RESID, EPI_SPLITK)

H16 = ["bf16", "f16"]
KINDS = ("tile", "glds", "direct")      # gcv_gemm_plan's kind codes (include/genconvit_hip.h)

# One launch as gcv_k_gemm takes it.  ptrs: one character each for A, Wt, C, bias, gamma, resid, partial: the byte offset
# from a 16-byte-aligned address as a hex digit, or - for a null pointer (the launcher looks at nullness and alignment only).
Launch = namedtuple("Launch", "a_mode epi M N K lda ldc act splitk kps H W cin_log2 cout_log2 ptrs")


def launch(a_mode, epi, M, N, K, lda=0, ldc=0, act=0, splitk=1, kps=0, H=0, W=0, cin_log2=0, cout_log2=0, bias=0, c_off=0,
           resid_off=0, **ptrs):
    p = {"A": 0, "Wt": 0, "C": None if epi == EPI_SPLITK else c_off, "bias": None if epi == EPI_SPLITK else bias,
         "gamma": 0 if epi == EPI_RESID else None, "resid": resid_off if epi == EPI_RESID else None,
         "partial": 0 if epi == EPI_SPLITK else None}
    p.update(ptrs)
    return Launch(a_mode, epi, M, N, K, lda, ldc, act, splitk, kps, H, W, cin_log2, cout_log2,
                  "".join("-" if p[k] is None else "%x" % p[k] for k in ("A", "Wt", "C", "bias", "gamma", "resid", "partial")))


def plan(dt, l):
    """gcv_gemm_plan of Launch l in storage dtype dt: (kind, five tile fields, grid.x, grid.y, threads, dynamic LDS bytes), or
    (rc, last error).  No GPU is needed."""
    import ctypes
    import torch
    from genconvit_amd import _lib
    p = [None if c == "-" else 0x100000 * (i + 1) + int(c, 16) for i, c in enumerate(l.ptrs)]      # never dereferenced
    g = _lib.GemmArgs(*p, l.M, l.N, l.K, l.lda, l.ldc, l.act, l.splitk, l.kps, l.H, l.W, l.cin_log2, l.cout_log2)
    out = (ctypes.c_int * 10)()
    dtype = {"f32": torch.float32, "f16": torch.float16, "bf16": torch.bfloat16}[dt]
    rc = _lib.load().gcv_gemm_plan(_lib.dtype_code(dtype), l.a_mode, l.epi, ctypes.byref(g), out)
    return (rc, _lib.last_error()) if rc else (KINDS[out[0]],) + tuple(out[1:])


def linear(M, N, K, act=ACT_NONE, ldc=None, **kw):
    return launch(A_PLAIN, EPI_BIAS_ACT, M, N, K, lda=K, ldc=N if ldc is None else ldc, act=act, **kw)


def resid(M, N, K, **kw):
    return launch(A_PLAIN, EPI_RESID, M, N, K, lda=K, ldc=N, **kw)


def splitk(M, N, K, nsplit, kps, **kw):
    return launch(A_PLAIN, EPI_SPLITK, M, N, K, lda=K, splitk=nsplit, kps=kps, **kw)


def conv_pool(n, H, cin, cout, ldc=None, **kw):
    return launch(A_IM2COL3_POOL, EPI_POOL4, n * H * H, cout, 9 * cin, ldc=ldc or cout, act=ACT_RELU, H=H, W=H,
                  cin_log2=cin.bit_length() - 1, **kw)


def conv_s2(n, H, cin, cout, ldc=None, **kw):
    return launch(A_IM2COL3_S2, EPI_BIAS_ACT, n * (H // 2) ** 2, cout, 9 * cin, ldc=ldc or cout, act=ACT_LEAKY, H=H, W=H,
                  cin_log2=cin.bit_length() - 1, **kw)


def conv_t(n, H, cin, cout, act, **kw):
    return launch(A_PLAIN, EPI_CONVT, n * H * H, 4 * cout, cin, lda=cin, act=act, H=H, W=H, cout_log2=cout.bit_length() - 1, **kw)


# ----------------------------------------------------------------------------- the kernels, as the lists below state them
# (kind, five tile fields) as gcv_gemm_plan reports them.  B: the default LDS row of the storage dtype (64 bytes = 16 k in
# fp32, 128 bytes = 64 k in 16 bit); K32: the 64-byte row of 16-bit launches with a short K tail (32 k).
_WAVE = {(32, 128): (32, 32), (64, 128): (32, 64), (128, 96): (32, 96), (128, 128): (64, 64), (128, 64): (32, 64),
         (128, 32): (32, 32)}


def tile(bm, bn, row="B"):
    return ("tile", bm, bn) + _WAVE[bm, bn] + (row,)


def dma(row):
    return ("glds", 128, 192, 64, 96, row)


def direct(cin, stride):
    return ("direct", cin, stride, 0, 0, 0)


K32 = 64


def resolve(kernel, dt):
    """the kernel a case states for storage dtype dt: (f32 kernel, 16-bit kernel) pairs, and the row B, resolved"""
    if isinstance(kernel[0], tuple):
        kernel = kernel[0 if dt == "f32" else 1]
    return tuple((64 if dt == "f32" else 128) if v == "B" else v for v in kernel)


def cases(lst):
    """the parameters of a list of (parameters, kernel) pairs, for pytest.mark.parametrize"""
    return [c for c, _ in lst]


# ----------------------------------------------------------------------------- tests/test_kernels_gpu.py
# test_gemm_bias_act (M, N, K, act), ldc = N + 8.  t128 = ceil(M / 128) * ceil(N / 128): 32 x 128 tiles below 48 (or M <= 32),
# 64 x 128 below 96 (or M <= 64), then 128 x 96 where N % 96 == 0, else 128 x 128.  16-bit launches with N % 192 == 0,
# K % 32 == 0, M >= 256 take the LDS-DMA kernel first.
BIAS_ACT = [
    ((300, 384, 96, 2), (tile(32, 128), dma(64))),       # ConvNeXt pw1 shape class, M tail, GELU: t128 = 9
    ((200, 1000, 768, 0), tile(32, 128)),                # head fc: N tail, t128 = 16
    ((40, 500, 2000, 2), tile(32, 128)),                 # GenConViT fc: N tail, t128 = 4
    ((8, 1000, 768, 1), tile(32, 128)),                  # M <= 32
    ((130, 192, 1536, 0), tile(32, 128)),                # downsample-conv shape class, long K (M < 256: not LDS-DMA)
    ((256, 96, 48, 3), tile(32, 128)),                   # K shorter than one 16-bit K tile
    ((9000, 384, 384, 2), (tile(128, 96), dma(64))),     # pw1 at K = 384 on the LDS-DMA kernel: 142 tiles + an M tail, GELU
    ((8200, 192, 384, 0), (tile(128, 96), dma(64))),     # ... one N tile, no activation
    ((70000, 1536, 384, 2), (tile(128, 96), dma(64))),   # ... the stage-2 shape class at full N: several rounds of workgroups
    # one case per tile that no launch above reaches: the smallest M, N with a ragged last M tile (and a ragged N tile where
    # the tile's rule allows one) and K of at least three K tiles
    ((40, 6144, 192, 2), tile(64, 128)),                 # t128 = 48, M <= 64
    ((130, 6100, 192, 1), tile(128, 128)),               # t128 = 96, N % 96 != 0
    ((130, 6240, 192, 3), (tile(128, 96), tile(128, 96))),      # t128 = 98, N % 96 == 0 (M < 256: not LDS-DMA in 16 bit)
    ((130, 6240, 96, 0), (tile(128, 96), tile(128, 96, K32))),  # ... K % 64 = 32: 32-deep K tiles in 16 bit
]


def bias_act_launch(M, N, K, act):
    return linear(M, N, K, act, ldc=N + 8)


# test_gemm_layerscale_residual (M, N, K): in place.  128 x 96 tiles where N % 96 == 0, else 128 x 128
RESID = [((300, 96, 384), tile(128, 96)), ((150, 256, 64), tile(128, 128)), ((129, 768, 3072), tile(128, 96))]

# test_gemm_splitk (M, N, K, splitk, k_per_split): 32 / 64 / 128 rows by M
SPLITK = [((8, 256, 512, 4, 128), tile(32, 128)), ((40, 384, 1024, 2, 512), tile(64, 128)), ((130, 128, 640, 3, 256), tile(128, 128))]

# test_conv3x3_relu_maxpool, test_conv3x3_stride2_leaky (n, H, cin, cout): 16-bit storage at Cin = 16 / 32 runs the direct
# kernel (stride 2: Cin = 16 only); N <= 32 / <= 64 / wider pick the tile, K = 144 / 288 the 32-deep K tile in 16 bit
CONV_POOL = [((2, 16, 16, 32), (tile(128, 32), direct(16, 1))), ((3, 8, 32, 64), (tile(128, 64), direct(32, 1))),
             ((2, 14, 128, 256), tile(128, 128)), ((1, 28, 64, 128), tile(128, 128)),
             ((3, 112, 16, 32), (tile(128, 32), direct(16, 1)))]     # 37632 rows: 294 tiles (256-row tiles were tried for such launches: 99 vs 79 us at B=128)
CONV_S2 = [((2, 16, 16, 32), (tile(128, 32), direct(16, 2))), ((3, 8, 32, 64), (tile(128, 64), tile(128, 64, K32))),
           ((2, 28, 64, 128), tile(128, 128))]
# the narrow tiles on 64-deep K tiles in 16 bit (Cin = 64: K = 576, nine K tiles) and the 128 x 64 tile on 32-deep ones
# (N = 48: not the direct kernel's): 300 rows, a ragged third M tile
CONV_POOL += [((3, 10, 64, 32), tile(128, 32)), ((3, 10, 64, 64), tile(128, 64)),
              ((3, 10, 16, 48), (tile(128, 64), tile(128, 64, K32)))]
CONV_S2 += [((3, 20, 64, 32), tile(128, 32)), ((3, 20, 64, 64), tile(128, 64))]

# test_conv_transpose_2x2 (n, H, cin, cout, act): N = 4 cout <= 64 the 128 x 64 tile
CONV_T = [((2, 7, 256, 128, 1), tile(128, 128)), ((3, 14, 64, 32, 3), tile(128, 128)), ((2, 28, 32, 16, 1), (tile(128, 64), tile(128, 64, K32))),
          ((3, 10, 192, 16, 3), tile(128, 64))]     # ... on 64-deep K tiles in 16 bit: K = 192, 300 rows

# test_gemm_at_one_and_three_rows_with_stage3_shapes: M in ROWS x (N, K) x both epilogues
STAGE3_ROWS = [1, 3]
STAGE3_NK = [(3072, 768), (768, 3072), (768, 1536)]
STAGE3_KERNEL = {"bias_gelu": tile(32, 128), "layerscale_residual": tile(128, 96)}

# test_gemm_lds_dma_pipeline_bias_act, ..._many_tiles_bias_act (M, N, K, act): the 128-byte-row ring where K % 64 == 0 and
# K >= 512, else the 64-byte-row ring
DMA_BIAS_ACT = [
    ((700, 1536, 384, 2), dma(64)),      # ConvNeXt stage-2 pw1 class (GELU)
    ((513, 192, 32, 0), dma(64)),        # one K tile  (pipeline shorter than the ring)
    ((256, 192, 64, 0), dma(64)),        # two K tiles
    ((300, 384, 96, 2), dma(64)),        # three K tiles, M tail
    ((384, 768, 128, 0), dma(64)),       # exactly ring depth
    ((1000, 384, 3072, 0), dma(128)),    # long K
]
DMA_BIAS_ACT_MANY = [((8229, 1536, 384, "gelu"), dma(64)), ((12544, 3072, 768, "gelu"), dma(128)), ((16400, 768, 128, "none"), dma(64))]
# test_gemm_lds_dma_pipeline_residual, ..._many_tiles_residual (M, N, K)
DMA_RESID = [((1000, 384, 1536), dma(128)), ((257, 768, 3072), dma(128)), ((640, 192, 768), dma(128))]
DMA_RESID_MANY = [((32868, 384, 1536), dma(128)), ((16500, 768, 3072), dma(128))]
# the 64-byte-row ring under the layer-scale epilogue: K below 512
DMA_RESID += [((300, 192, 96), dma(64))]

# ----------------------------------------------------------------------------- tests/test_conv_direct_gpu.py
# (n, H, cin, cout); ldc = cout + PAD, the result GUARD rows into its buffer (16-byte aligned, asserted there)
DIRECT_PAD, DIRECT_GUARD = 8, 4
DIRECT_POOL = [((1, 2, 16, 32), direct(16, 1)), ((3, 6, 16, 32), direct(16, 1)), ((3, 6, 32, 64), direct(32, 1)),
               ((2, 16, 32, 64), direct(32, 1)), ((2, 16, 16, 16), tile(128, 32, K32))]
DIRECT_S2 = [((1, 2, 32, 64), tile(128, 64, K32)), ((5, 6, 16, 32), direct(16, 2)), ((5, 6, 32, 64), tile(128, 64, K32)),
             ((2, 16, 16, 16), tile(128, 32, K32))]


def direct_launch(mode, n, H, cin, cout):
    ldc = cout + DIRECT_PAD
    return (conv_pool if mode == "pool" else conv_s2)(n, H, cin, cout, ldc=ldc, c_off=DIRECT_GUARD * ldc * 2 % 16)


# ----------------------------------------------------------------------------- tests/test_numerics_gpu.py
# (name, storage dtypes, M, N = K, ldc), GELU: one site per tile of the plain bias + activation launch and the LDS-DMA kernel.
# N = 128 / 96 and an ldc that is no multiple of 8 keep the 16-bit launches off the LDS-DMA kernel.  M is never a multiple of
# the tile.
GELU_SITES = [
    (("f32", ["f32"], 1021, 128, 128), tile(32, 128)),    # fp32 storage: act_fn / erf_fast
    (("C1", H16, 517, 128, 128), tile(32, 128)),          # t128 = 5
    (("C2", H16, 6200, 128, 128), tile(64, 128)),         # t128 = 49
    (("C3S", H16, 12300, 96, 96), tile(128, 96, K32)),    # t128 = 97, N % 96 == 0, K % 64 = 32
    (("C3", H16, 6200, 192, 196), tile(128, 96)),         # t128 = 98, N % 96 == 0, K % 64 == 0 (ldc 196: not LDS-DMA)
    (("C4", H16, 12300, 128, 128), tile(128, 128)),       # t128 = 97
    (("glds", H16, 331, 192, 192), dma(64)),              # N = 192, M >= 256, everything 16-byte aligned
]

# ----------------------------------------------------------------------------- tests/test_cam_kernels_gpu.py
# test_backward_contraction_gemm_with_one_split (N, K) at CAM_ROWS rows
CAM_ROWS = 13
CAM_CONTRACTION = [((3072, 768), tile(32, 128)), ((768, 3072), tile(32, 128))]


def gpu_launches(dt):
    """every (Launch, stated kernel) that the GPU tests run in storage dtype dt"""
    h16 = dt != "f32"
    out = [(bias_act_launch(*c), k) for c, k in BIAS_ACT]
    out += [(resid(*c), k) for c, k in RESID]
    out += [(splitk(*c), k) for c, k in SPLITK]
    out += [(conv_pool(*c), k) for c, k in CONV_POOL] + [(conv_s2(*c), k) for c, k in CONV_S2]
    out += [(conv_t(*c), k) for c, k in CONV_T]
    for M in STAGE3_ROWS:
        for N, K in STAGE3_NK:
            out += [(linear(M, N, K, ACT_GELU), STAGE3_KERNEL["bias_gelu"]), (resid(M, N, K), STAGE3_KERNEL["layerscale_residual"])]
    out += [(splitk(CAM_ROWS, N, K, 1, K), k) for (N, K), k in CAM_CONTRACTION]
    out += [(linear(M, N, N, ACT_GELU, ldc=ldc), k) for (_, dts, M, N, ldc), k in GELU_SITES if dt in dts]
    if h16:
        out += [(linear(*c), k) for c, k in DMA_BIAS_ACT]
        out += [(linear(M, N, K, {"none": ACT_NONE, "gelu": ACT_GELU}[a]), k) for (M, N, K, a), k in DMA_BIAS_ACT_MANY]
        out += [(resid(*c), k) for c, k in DMA_RESID + DMA_RESID_MANY]
        out += [(direct_launch("pool", *c), k) for c, k in DIRECT_POOL] + [(direct_launch("s2", *c), k) for c, k in DIRECT_S2]
    return out


# ----------------------------------------------------------------------------- the networks' launches, by formula
CNX_DIMS = {"tiny": (96, 192, 384, 768), "large": (192, 384, 768, 1536)}
BATCHES = (1, 32, 33, 64, 67, 128, 256)


def _backbone(dims, toks, head_rows, head_ldc, head_act, explain=True):
    """a ConvNeXt pass over toks[i] tokens at stage i: the down-sampling convs, the MLP as two GEMMs (MlpKind::Gemm, cnx_mlp.h)
    and the classifier; explain: the classifier's pre-activation copy and the four contractions of explain at stage 2"""
    out = []
    for i, C in enumerate(dims):
        if i:
            out.append(linear(toks[i], C, 4 * dims[i - 1]))
        out += [linear(toks[i], 4 * C, C, ACT_GELU), resid(toks[i], C, 4 * C)]
    C2, C3 = dims[2], dims[3]
    out.append(linear(head_rows, 1000, C3, head_act, ldc=head_ldc))
    if explain:
        out += [linear(head_rows, 1000, C3, ACT_NONE, ldc=head_ldc), splitk(toks[3], 4 * C3, C3, 1, C3),
                linear(toks[3], 4 * C3, C3), splitk(toks[3], C3, 4 * C3, 1, 4 * C3), splitk(toks[3], 4 * C2, C3, 1, C3)]
    return out


def network_launches(arch, B):
    """every launch_gemm call of the ED and VAE networks (net_impl.h, both VAE schedules), their explain passes and Swin-T
    (swin.h) at B frames; operands 256-byte aligned, as the arena gives them"""
    dims = CNX_DIMS[arch]
    out = []
    # ED: encoder convs + pool, decoder transposed convs, both backbone passes as one 2B-image stream, the head's split-K fc
    out += [conv_pool(B, H, 1 << cl, 2 << cl) for H, cl in zip((112, 56, 28, 14), (4, 5, 6, 7))]
    out += [conv_t(B, H, 2 << col, 1 << col, ACT_RELU) for H, col in zip((7, 14, 28, 56), (7, 6, 5, 4))]
    out += _backbone(dims, [2 * B * (56 >> i) ** 2 for i in range(4)], 2 * B, 1000, ACT_GELU)
    out.append(splitk(B, 500, 2000, 8, 256))
    # VAE: stride-2 encoder convs, mu / var split 7 ways up to 64 frames and 8 ways above, decoder; the 224- and the 112-pixel
    # pass as one stream, or one stream each (the split schedule: classifier rows into the (B, 2000) feature matrix)
    out += [conv_s2(B, H, 1 << cl, 2 << cl) for H, cl in zip((112, 56, 28), (4, 5, 6))]
    nsplit = 7 if B <= 64 else 8
    out.append(splitk(B, 12544, 25088, nsplit, 25088 // nsplit))
    out += [conv_t(B, H, cin, 1 << col, ACT_LEAKY) for H, cin, col in zip((7, 14, 28), (256, 64, 32), (6, 5, 4))]
    out += _backbone(dims, [B * ((56 >> i) ** 2 + (28 >> i) ** 2) for i in range(4)], 2 * B, 1000, ACT_RELU)
    for side in (56, 28):
        out += _backbone(dims, [B * (side >> i) ** 2 for i in range(4)], B, 2000, ACT_RELU, explain=False)
    # Swin-T
    for i, C in enumerate((96, 192, 384, 768)):
        M = B * (56 >> i) ** 2
        out += [linear(M, 3 * C, C), resid(M, C, C), linear(M, 4 * C, C, ACT_GELU), resid(M, C, 4 * C)]
        if i < 3:
            out.append(linear(M // 4, 2 * C, 4 * C, bias=None))
    out.append(linear(B, 1000, 768))
    return out


# ----------------------------------------------------------------------------- alignment rules and errors
# one launch per alignment rule that changes the kernel (16-bit storage: the LDS-DMA and the direct kernel store 16 bytes at
# a time), next to the aligned launch
ALIGNMENT = [linear(512, 192, 384), linear(512, 192, 384, c_off=8), linear(512, 192, 384, ldc=196),
             resid(512, 192, 768), resid(512, 192, 768, c_off=8, resid_off=8), resid(512, 192, 768, resid_off=4),
             conv_s2(2, 16, 16, 32), conv_s2(2, 16, 16, 32, c_off=8), conv_s2(2, 16, 16, 32, ldc=36),
             conv_pool(2, 16, 16, 32, c_off=8), conv_pool(2, 16, 16, 32, ldc=36), conv_pool(2, 16, 16, 32, bias=None)]

# one launch per error of the launcher: (Launch, text of the error)
ERRORS = [
    (linear(0, 64, 64), "empty GEMM"),
    (linear(8, 64, 66), "K must be a multiple of the 16-byte chunk"),
    (linear(8, 66, 64), "N must be a multiple of 4"),
    (linear(8, 64, 64, A=2), "A/Wt must be 16-byte aligned"),
    (linear(8, 64, 64, Wt=8), "A/Wt must be 16-byte aligned"),
    (linear(8, 64, 64, C=None), "C must be aligned to 4 elements"),
    (linear(8, 64, 64, c_off=2), "C must be aligned to 4 elements"),
    (linear(8, 64, 64, ldc=60), "ldc must be a multiple of 4 and >= N"),
    (linear(8, 64, 64, ldc=66), "ldc must be a multiple of 4 and >= N"),
    (linear(8, 64, 64, bias=8), "bias must be 16-byte aligned"),
    (linear(8, 64, 64)._replace(lda=56), "lda must be a chunk multiple >= K"),
    (conv_pool(2, 16, 16, 32)._replace(K=128), "im2col: K = 9*Cin, Cin chunk-aligned"),
    (conv_pool(2, 16, 16, 32)._replace(W=15), "im2col modes need even H, W"),
    (splitk(8, 64, 512, 0, 512), "bad split-K plan"),
    (splitk(8, 64, 512, 2, 128), "bad split-K plan"),
    (splitk(8, 64, 512, 2, 264), "bad split-K plan"),
    (splitk(8, 64, 512, 2, 256, partial=None), "bad split-K plan"),
    (resid(8, 64, 64, gamma=None), "EPI_RESID needs gamma and resid"),
    (resid(8, 64, 64, resid=None), "EPI_RESID needs gamma and resid"),
    (conv_pool(2, 16, 16, 32)._replace(M=510), "EPI_POOL4 needs M % 4 == 0"),
    (conv_t(2, 7, 64, 32, ACT_RELU)._replace(N=64), "EPI_CONVT shape"),
    (conv_t(2, 7, 64, 32, ACT_RELU)._replace(M=97), "EPI_CONVT shape"),
    (linear(8, 64, 64, act=7), "bad activation code"),
    (resid(8, 64, 64)._replace(act=ACT_GELU), "EPI_RESID has no activation"),
    (conv_t(2, 7, 64, 32, ACT_GELU), "EPI_CONVT is built for ReLU / LeakyReLU"),
    (conv_pool(2, 16, 16, 32)._replace(act=ACT_LEAKY), "conv3x3+pool is built for ReLU"),
    (conv_s2(2, 16, 16, 32)._replace(act=ACT_RELU), "conv3x3 stride 2 is built for LeakyReLU"),
    (conv_pool(2, 16, 16, 32)._replace(epi=EPI_BIAS_ACT), "unsupported (a_mode, epilogue) combination"),
    (linear(8, 64, 64)._replace(epi=EPI_POOL4), "unsupported (a_mode, epilogue) combination"),
]


def table_launches():
    """every Launch that tests/golden/gemm_plan.json pins, in any storage dtype"""
    need = {l for arch in CNX_DIMS for B in BATCHES for l in network_launches(arch, B)}
    need |= {l for dt in ("f32", "f16") for l, _ in gpu_launches(dt)}
    return need | set(ALIGNMENT) | {l for l, _ in ERRORS}
