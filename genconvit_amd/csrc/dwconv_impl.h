// The depthwise 7x7 + LayerNorm of the ConvNeXt block (run tag cnx.dwconv7_ln): dw_select picks one of its six kernels and
// plans its grid, launch_dwconv7_ln launches from that plan.  Included by dw_{f32,f16,bf16}.hip, which compile the band
// kernels with -fno-slp-vectorize: left alone, hipcc packs the rolling kernel's tap FMAs into v_pk_fma_f32 (no faster than
// two v_fma_f32 on gfx950) whose even-aligned register pairs cost ~290 spilled registers.  The tile kinds are compiled in
// kern_{f32,f16,bf16}.hip (kernels_impl.h, launch_dw_tile).
#pragma once
#include <algorithm>
#include <type_traits>

#include "dwconv_mfma.h"
#include "dwconv_pair.h"
#include "dwconv_roll.h"
#include "kernels.h"

namespace gcv {

// 16-bit C = 96 / 56-pixel launches of at least this many image rows (images x H) run the matrix-pipe kernel
constexpr int64_t kDwMfmaMinImageRows = 14 * 256;

// a kernel of dw_select; C and N = NS: the template shape of a band kind (tile kinds: 0, their shape is in the plan)
template <DwKind K, int C_ = 0, int N_ = 0> struct DwShape {
  static constexpr DwKind kind = K;
  static constexpr int C = C_, N = N_;
};

// The launch of nimg images of H x W x C, x and y 16-byte `aligned` or not.  The kernel, in order of precedence:
//   1. aligned maps W = 7 NS pixels wide: a band kernel, one workgroup per (image, band of rows) across the whole width.
//      Roll (dwconv_roll.h, rolling strips) where NS * C <= 768, Pair (dwconv_pair.h, two channels per lane) where
//      NS * C = 1536, the 224-pixel stages of ConvNeXt-L.  At C = 96 / 56 pixels in 16-bit storage, Mfma (dwconv_mfma.h)
//      runs the taps on the matrix pipe for launches of 64 images and more, whose bands are at least 14 rows long: a
//      workgroup first zeroes its ring and builds 42 tap-operand registers per lane from 84 global loads, which a 7-row band
//      does not pay back (vae B = 32 bf16, paired runs: 19.3k fps with it, 19.9k with Roll).  Mfma is also correct at
//      C = 96 / 28 pixels and C = 192 / 28, 14 pixels, but inside the step those launches were 9 - 33 % slower than Roll
//      (DESIGN.md §4.1 item 11).
//   2. S x S maps, S <= 4: one workgroup per image, Tiny at C = 768, TinyPair (two channels per lane) at C = 1536.
//   3. Tile, the generic tile kernel, at C <= 768.
// Every kernel is reachable: gcv_convnext_forward takes res = 32 ... 224 in steps of 4, so the stage-3 map can be 1 x 1 to
// 4 x 4 (all four S of Tiny and TinyPair), and maps whose width is not a multiple of 7 (res 160: 5 x 5 at stage 3) or
// unaligned operands reach Tile.  There is no Tile kernel at C = 1536: a 5- or 6-pixel map there (ConvNeXt-L at res
// 160 ... 220) is this function's error, which is why cnx_res_ok (net.h) refuses those resolutions before the pass starts.
// Every (kind, C, NS or S) returned here has a GPU parity case (tests/dwcases.py; tests/test_host_cpu.py checks the set).
// Calls f(plan, DwShape) and returns its value, or sets the launcher's error.
template <typename T, class F> int dw_select(int nimg, int H, int W, int C, bool aligned, F&& f) {
  GCV_REQUIRE(nimg > 0 && H > 0 && W > 0, "dwconv: empty");
  const int ns = W % 7 == 0 ? W / 7 : 0;
  auto go = [&](auto sh) -> int {
    typedef decltype(sh) S;
    DwPlan p;
    p.kind = S::kind; p.C = C;
    if constexpr (S::kind == DwKind::Tile) {
      const int tiles = C == 96 ? 2 : 1;                                 // as dwconv7_ln_kernel
      p.block = tiles * C;
      p.lds = tiles * 49 * (C + 2) * 4;
      p.grid = cdiv(nimg * cdiv(H, 7) * cdiv(W, 7), tiles);
    } else if constexpr (S::kind == DwKind::Tiny || S::kind == DwKind::TinyPair) {
      p.n = H; p.block = 768; p.grid = nimg;                            // 768 lanes of one channel (Tiny) or two
    } else {
      GCV_REQUIRE((int64_t)H * W * C * (int64_t)sizeof(T) < (int64_t)1 << 31, "dwconv: one image must stay below 2 GiB");
      int nb;
      if constexpr (S::kind == DwKind::Pair) {
        p.block = kDwPairThreads;
        nb = std::max(1, std::min(H, (512 + nimg - 1) / nimg));          // two workgroups per CU
      } else {
        typedef std::conditional_t<S::kind == DwKind::Mfma, DwMfmaLds<T, S::C, S::N>, DwRollLds<T, S::C, S::N>> LY;
        p.block = LY::NT;
        p.lds = LY::bytes;
        // bands: enough workgroups to fill 256 CUs (116 VGPRs: 16 waves per CU), never fewer than 7 output rows per band
        // unless the image itself is smaller (each band re-reads a 6-row input apron) ... except for launches that 7-row
        // bands would spread over at most half the CUs (batches of 32, the 112-pixel pass): there a band's walk of rows + 6
        // steps at ~2 us each IS the launch time, so bands shrink to as little as two rows (8 steps instead of 13; the
        // re-read aprons come from L2)
        const int per_cu = std::max(1, std::min(160 * 1024 / LY::bytes, LY::NT > 512 ? 1 : 2));
        const int nb7 = std::max(1, H / 7);
        const bool small_launch = nimg * nb7 <= 128;
        nb = std::max(1, std::min((256 * per_cu + nimg - 1) / nimg, small_launch ? std::max(1, H / 2) : nb7));
      }
      p.n = ns;
      p.band_rows = cdiv(H, nb);
      p.grid = nimg * cdiv(H, p.band_rows);
    }
    return f(p, sh);
  };
  if (aligned) {
    switch (C) {
      case 96:
        if constexpr (sizeof(T) == 2)
          if (ns == 8 && (int64_t)nimg * H >= kDwMfmaMinImageRows) return go(DwShape<DwKind::Mfma, 96, 8>{});
        if (ns == 8) return go(DwShape<DwKind::Roll, 96, 8>{});
        if (ns == 4) return go(DwShape<DwKind::Roll, 96, 4>{});
        break;
      case 192:
        if (ns == 4) return go(DwShape<DwKind::Roll, 192, 4>{});
        if (ns == 2) return go(DwShape<DwKind::Roll, 192, 2>{});
        if (ns == 8) return go(DwShape<DwKind::Pair, 192, 8>{});
        break;
      case 384:
        if (ns == 2) return go(DwShape<DwKind::Roll, 384, 2>{});
        if (ns == 1) return go(DwShape<DwKind::Roll, 384, 1>{});
        if (ns == 4) return go(DwShape<DwKind::Pair, 384, 4>{});
        break;
      case 768:
        if (ns == 1) return go(DwShape<DwKind::Roll, 768, 1>{});
        if (ns == 2) return go(DwShape<DwKind::Pair, 768, 2>{});
        break;
      case 1536:
        if (ns == 1) return go(DwShape<DwKind::Pair, 1536, 1>{});
        break;
    }
  }
  if (H == W && H <= 4 && C == 768) return go(DwShape<DwKind::Tiny>{});
  if (H == W && H <= 4 && C == 1536) return go(DwShape<DwKind::TinyPair>{});
  if (C == 96 || C == 192 || C == 384 || C == 768) return go(DwShape<DwKind::Tile>{});
  set_error("dwconv7_ln: C must be one of 96/192/384/768 (1536: 7-pixel-wide maps, or up to 4 x 4, only)");
  return -3;
}

template <typename T> int dw_plan(DwPlan& p, int nimg, int H, int W, int C, bool aligned) {
  return dw_select<T>(nimg, H, W, C, aligned, [&](const DwPlan& q, auto) { p = q; return 0; });
}

template <typename T>
int launch_dwconv7_ln(const T* x, const float* wdw, const float* bdw, const float* lnw, const float* lnb, T* y,
                      int nimg, int H, int W, int C, float eps, hipStream_t s) {
  const bool aligned = ((reinterpret_cast<uintptr_t>(x) | reinterpret_cast<uintptr_t>(y)) & 15u) == 0;
  return dw_select<T>(nimg, H, W, C, aligned, [&](const DwPlan& p, auto sh) -> int {
    typedef decltype(sh) S;
    auto band = [&](auto k) {
      return dw_launch(p, k, s, x, wdw, bdw, lnw, lnb, y, H, p.band_rows, cdiv(H, p.band_rows), eps);
    };
    if constexpr (S::kind == DwKind::Roll) return band(dwconv7_ln_roll_kernel<T, S::C, S::N>);
    else if constexpr (S::kind == DwKind::Mfma) return band(dwconv7_ln_mfma_kernel<T, S::C, S::N>);
    else if constexpr (S::kind == DwKind::Pair) return band(dwconv7_ln_pair_kernel<T, S::C, S::N>);
    else return launch_dw_tile<T>(p, x, wdw, bdw, lnw, lnb, y, nimg, H, W, eps, s);
  });
}

#define GCV_INSTANTIATE_DW(T)                                                                                        \
  template int dw_plan<T>(DwPlan&, int, int, int, int, bool);                                                        \
  template int launch_dwconv7_ln<T>(const T*, const float*, const float*, const float*, const float*, T*, int, int,   \
                                    int, int, float, hipStream_t);

}  // namespace gcv
