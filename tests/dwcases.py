"""The (C, H, W, n) shapes of the GPU parity tests of the depthwise 7x7 + LayerNorm (gcv_k_dwconv7_ln), in one place: the
GPU tests parametrise over these lists, and tests/test_host_cpu.py asks gcv_dw_plan, without a GPU, which kernel each of
them runs — every kernel dw_select (csrc/dwconv_impl.h) can return must be the plan of at least one shape here, and every
band geometry that a batch of the networks reaches the plan of one entry of GEOMETRY / MERGED below."""

# tests/test_kernels_gpu.py: test_dwconv7x7_layernorm (square maps, (C, H, n))
SQUARE = [(96, 56, 2), (96, 28, 3), (192, 28, 2), (192, 14, 1), (384, 14, 2), (384, 7, 3),
          (768, 7, 2), (768, 3, 3),
          (768, 1, 5), (768, 2, 3), (768, 4, 2),      # whole-map kernel of the tiny stage-3 maps (with (768, 3, 3))
          # launches of more than 128 seven-row bands keep seven-row bands (the large-batch rule);
          # the few-image cases above run the two- to four-row bands of small launches
          (96, 56, 17), (384, 14, 70),
          # 16-bit storage, 56-pixel C = 96 maps in bands of 14 rows and more: the matrix-pipe kernel
          # (dwconv_mfma.h; fp32 storage stays on the VALU kernel): four 14-row bands, ragged 19/19/18
          (96, 56, 64), (96, 56, 100)]

# tests/test_large_gpu.py: test_dwconv7x7_layernorm_large_shapes ((C, H, n); (1536, 2, n): TinyPair S = 2, ConvNeXt-L at
# res 64 ... 92)
LARGE = [(192, 56, 3), (384, 28, 3), (768, 14, 5), (1536, 7, 3), (1536, 7, 600),
         (1536, 3, 3), (1536, 1, 2), (1536, 4, 2), (1536, 2, 3)]

# The generic tile kernel (DwKind::Tile, dwconv7_ln_kernel<T, C>): maps whose width is not 7 NS of a band kernel.
# (C, H, W, n): 5, 6, 10, 20, 40 are the maps of a res-160 pass; 9 and 25 are odd with ragged right / bottom 7x7 tiles (2 x 2
# and 4 x 4 tiles); one non-square map and one single-row map.
TILE = [(C, H, W, n) for C in (96, 192, 384, 768)
        for H, W, n in [(5, 5, 3), (6, 6, 2), (10, 10, 2), (20, 20, 2), (40, 40, 2), (9, 9, 2), (25, 25, 1), (10, 25, 2),
                        (1, 13, 3)]]
TILE += [(96, 14, 14, 2),      # res 56 at C = 96: 14 = 7 * 2 but there is no two-strip kernel at 96 channels
         (96, 9, 9, 1),        # C = 96 packs two tiles per workgroup: 4 tiles, both slots busy in both workgroups
         (96, 25, 25, 3)]      # 48 tiles
# at C = 96 an odd tile count leaves the second tile slot of the last workgroup idle (tile_ok == false): (96, 5, 5, 3) above
# is 3 tiles; these are 1, 3 (non-square) and 9
TILE_ODD = [(96, 5, 5, 1), (96, 5, 15, 1), (96, 20, 20, 1)]

# Band kernels (Roll / Mfma / Pair) away from squares: H != W, H < 7, H not a multiple of the band.  (C, H, W, n)
BANDS = [(96, 1, 56, 3), (96, 5, 56, 2), (96, 57, 56, 2),      # Roll<96, 8>
         (96, 57, 56, 63),      # 3 591 image rows: Mfma<96, 8> in 16-bit storage (8-row bands, the last band one row)
         (96, 5, 56, 717),      # 3 585 image rows of 5-row images: Mfma with a band shorter than the 7 tap rows
         (96, 9, 28, 3), (192, 3, 28, 2), (192, 30, 14, 2), (384, 15, 14, 3), (384, 2, 7, 4), (768, 10, 7, 3),   # other Roll shapes
         (192, 30, 56, 2), (384, 13, 28, 2), (768, 9, 14, 3), (1536, 5, 7, 3), (1536, 16, 7, 2)]      # Pair, H != W


# ---- launch geometry.  A band kernel's rows per band (and Mfma against Roll at C = 96 / 56 pixels) follow from the image count
# of the launch, so the few-image cases above run the small-launch bands only.  gcv_k_dwconv7_ln_planned launches n images
# under the plan of plan_nimg images.  GEOMETRY is one (C, H, plan_nimg) per (kind, C, NS, H, band_rows) that ConvNeXt-T or
# ConvNeXt-L reach at any batch of any network (tests/census.py walks them through gcv_dw_plan; tests/test_host_cpu.py
# asserts that the keys reached and the keys of this list are the same set per storage dtype), plan_nimg the smallest count
# with that key.  H x H maps, n = 2 (tests/test_kernels_gpu.py: test_dwconv7x7_layernorm_at_every_band_geometry).
GEOMETRY = [
    (96, 28, 1), (96, 28, 33), (96, 28, 171), (96, 28, 256), (96, 28, 512),
    # 56 pixels at C = 96: from 64 images on, Mfma in 16-bit storage and Roll in fp32, at the same rows per band
    (96, 56, 1), (96, 56, 10), (96, 56, 15), (96, 56, 17), (96, 56, 37), (96, 56, 43), (96, 56, 52), (96, 56, 64), (96, 56, 86),
    (96, 56, 128), (96, 56, 256),
    (192, 14, 1), (192, 14, 65), (192, 14, 512),
    (192, 28, 1), (192, 28, 20), (192, 28, 29), (192, 28, 33), (192, 28, 86), (192, 28, 128), (192, 28, 256),
    # Pair<192, 8>: stage 0 of ConvNeXt-L, one row per band up to 9 images, the whole map from 512 on
    (192, 56, 1), (192, 56, 10), (192, 56, 19), (192, 56, 29), (192, 56, 40), (192, 56, 47), (192, 56, 57), (192, 56, 74),
    (192, 56, 86), (192, 56, 103), (192, 56, 128), (192, 56, 171), (192, 56, 256), (192, 56, 512),
    (384, 7, 1), (384, 7, 129),
    (384, 14, 1), (384, 14, 43), (384, 14, 64), (384, 14, 65), (384, 14, 256),
    (384, 28, 1), (384, 28, 19), (384, 28, 40), (384, 28, 57), (384, 28, 86), (384, 28, 103), (384, 28, 128), (384, 28, 171),
    (384, 28, 256), (384, 28, 512),                                                                     # Pair<384, 4>
    (768, 7, 1), (768, 7, 128), (768, 7, 129),
    (768, 14, 1), (768, 14, 40), (768, 14, 86), (768, 14, 128), (768, 14, 171), (768, 14, 256), (768, 14, 512),   # Pair<768, 2>
    (1536, 7, 1), (1536, 7, 86), (1536, 7, 171), (1536, 7, 256), (1536, 7, 512),                        # Pair<1536, 1>
]
# three images, once per band kernel: the entry with its second-smallest plan_nimg (more than one band of more than one row)
GEOMETRY_N3 = [(96, 28, 33), (96, 56, 10), (96, 56, 86), (192, 14, 65), (192, 28, 20), (192, 56, 10), (384, 7, 129), (384, 14, 43),
               (384, 28, 19), (768, 7, 128), (768, 14, 40), (1536, 7, 86)]

# The merged two-group launch (launch_dwconv7_ln2): every pair of keys that the VAE's merged 224- + 112-pixel pass reaches on
# ConvNeXt-T, as (C, H0, H1, plan_nimg0, plan_nimg1) at the smallest batch with that pair (tests/test_dw_merged_gpu.py; the
# census of tests/test_host_cpu.py again).  ConvNeXt-L has no merged pair.
MERGED = [
    (192, 28, 14, 1, 1), (192, 28, 14, 20, 20), (192, 28, 14, 29, 29), (192, 28, 14, 33, 33), (192, 28, 14, 65, 65),
    (192, 28, 14, 86, 86), (192, 28, 14, 128, 128), (192, 28, 14, 256, 256), (192, 28, 14, 512, 512),
    (384, 14, 7, 1, 1), (384, 14, 7, 43, 43), (384, 14, 7, 64, 64), (384, 14, 7, 65, 65), (384, 14, 7, 129, 129),
    (384, 14, 7, 256, 256),
    (768, 7, 3, 1, 1), (768, 7, 3, 128, 128), (768, 7, 3, 129, 129),
]


def all_cases():
    """every (C, H, W, n) above"""
    sq = [(C, H, H, n) for C, H, n in SQUARE + LARGE]
    return sq + TILE + TILE_ODD + BANDS


# the kernels dw_select can return, as (kind, C, NS or S) — kind as tests/test_host_cpu.py names gcv_dw_plan's codes
ROLL = {("roll", 96, 8), ("roll", 96, 4), ("roll", 192, 4), ("roll", 192, 2), ("roll", 384, 2), ("roll", 384, 1),
        ("roll", 768, 1)}
MFMA = {("mfma", 96, 8)}                               # 16-bit storage only
PAIR = {("pair", 192, 8), ("pair", 384, 4), ("pair", 768, 2), ("pair", 1536, 1)}
TINY = {("tiny", 768, s) for s in (1, 2, 3, 4)} | {("tiny_pair", 1536, s) for s in (1, 2, 3, 4)}
TILES = {("tile", C, 0) for C in (96, 192, 384, 768)}


def reachable(dt):
    return ROLL | PAIR | TINY | TILES | (MFMA if dt != "f32" else set())
