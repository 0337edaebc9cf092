// The depthwise 7x7 + LayerNorm of the ConvNeXt block (run tag cnx.dwconv7_ln): dw_select picks one of its six kernels and
// plans its grid, launch_dwconv7_ln launches from that plan, launch_dwconv7_ln2 two such plans in one grid.  Included by dw_{f32,f16,bf16}.hip, which compile the band
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
#include "kernels_dev.h"

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
// Every (kind, C, NS or S) returned here has a GPU parity case (tests/dwcases.py; tests/test_host_cpu.py checks the set),
// and so has every (band kernel, H, rows per band) that a batch of the networks reaches (tests/census.py).
// Calls f(plan, DwShape) and returns its value, or sets the launcher's error.
// plan_nimg > 0 (the kernel-test entries gcv_k_dwconv7_ln*_planned): the kernel and the rows per band are those of a launch
// of plan_nimg images, the grid covers nimg images; every network launch plans on its own count.
template <typename T, class F> int dw_select(int nimg, int H, int W, int C, bool aligned, F&& f, int plan_nimg = 0) {
  GCV_REQUIRE(nimg > 0 && H > 0 && W > 0, "dwconv: empty");
  const int pn = plan_nimg > 0 ? plan_nimg : nimg;
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
        nb = std::max(1, std::min(H, (512 + pn - 1) / pn));              // two workgroups per CU
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
        const bool small_launch = (int64_t)pn * nb7 <= 128;
        nb = std::max(1, std::min((256 * per_cu + pn - 1) / pn, small_launch ? std::max(1, H / 2) : nb7));
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
          if (ns == 8 && (int64_t)pn * H >= kDwMfmaMinImageRows) return go(DwShape<DwKind::Mfma, 96, 8>{});
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
                      int nimg, int H, int W, int C, float eps, hipStream_t s, int plan_nimg) {
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
  }, plan_nimg);
}

// ---- two image groups in one launch (the 224- and the 112-pixel segment of the VAE's merged backbone pass) ----
// Each group keeps the kernel, bands and grid dw_select plans for it alone; the two grids are laid end to end and a workgroup
// runs the body of the group its index falls into, so every image's bands are computed by the device code of the
// single-group launch under the same plan.  The launch takes the larger block and the larger LDS of the two; the waves the
// smaller body has no use for return before its first barrier.
template <typename T> struct DwGroupArgs {
  const T* x;
  T* y;
  int H, band_rows, nbands;
};

// the body of a kind as a device function of (LDS base, workgroup index, workgroups of its group)
template <typename T, class S> struct DwBody;
template <typename T, int C, int N> struct DwBody<T, DwShape<DwKind::Roll, C, N>> {
  static constexpr int NT = DwRollLds<T, C, N>::NT, lds = DwRollLds<T, C, N>::bytes;
  __device__ static __forceinline__ void run(unsigned char* l, int bid, int nwg, const DwGroupArgs<T>& a, const float* wdw,
                                             const float* bdw, const float* lnw, const float* lnb, float eps) {
    dwconv7_ln_roll_body<T, C, N>(l, bid, nwg, a.x, wdw, bdw, lnw, lnb, a.y, a.H, a.band_rows, a.nbands, eps);
  }
};
template <typename T, int C, int N> struct DwBody<T, DwShape<DwKind::Mfma, C, N>> {
  static constexpr int NT = DwMfmaLds<T, C, N>::NT, lds = DwMfmaLds<T, C, N>::bytes;
  __device__ static __forceinline__ void run(unsigned char* l, int bid, int nwg, const DwGroupArgs<T>& a, const float* wdw,
                                             const float* bdw, const float* lnw, const float* lnb, float eps) {
    dwconv7_ln_mfma_body<T, C, N>(l, bid, nwg, a.x, wdw, bdw, lnw, lnb, a.y, a.H, a.band_rows, a.nbands, eps);
  }
};
template <typename T, int C, int S> struct DwBody<T, DwShape<DwKind::Tiny, C, S>> {
  static constexpr int NT = C, lds = 0;              // its partial sums are static LDS, in front of the dynamic block
  __device__ static __forceinline__ void run(unsigned char*, int bid, int, const DwGroupArgs<T>& a, const float* wdw,
                                             const float* bdw, const float* lnw, const float* lnb, float eps) {
    dwconv7_ln_tiny_body<T, C, S>(bid, a.x, wdw, bdw, lnw, lnb, a.y, eps);
  }
};

// The pairs with a merged kernel, group 0 the wider map: stages 1 - 3 of ConvNeXt-T's 224- + 112-pixel pass.
//   Roll<192,4> + Roll<192,2>,  Roll<384,2> + Roll<384,1>,  Roll<768,1> + Tiny<768,3>
// Stage 0, (Mfma<96,8> | Roll<96,8>) + Roll<96,4>, keeps two launches: all three kernels sit at the 128 registers of a
// 16-wave workgroup (Roll<96,4> with one dword of scratch, isa_report.py), and either merged kernel came out with a
// second spilled register, the thread index carried across the tap waves' loop for the staging waves.
// Tiny at S = 3 only: a two-segment pass is the VAE's, whose maps are 7 and 7 / 2 = 3 pixels at stage 3, and no other
// resolution that cnx_res_ok accepts puts a 7-pixel map beside a 1-, 2- or 4-pixel one.  Everything else (Tile, Pair,
// TinyPair, unaligned operands, ConvNeXt-L, groups in the other order) keeps two launches as well.
template <class S0, class S1> constexpr bool dw_two_roll_pair() {
  return S0::kind == DwKind::Roll && S1::kind == DwKind::Roll && S0::C == S1::C && S0::N == 2 * S1::N &&
         S0::N * S0::C == 768 && S0::C != 96;
}
template <class S0> constexpr bool dw_two_tiny_pair() { return S0::kind == DwKind::Roll && S0::C == 768 && S0::N == 1; }
constexpr int kDwTwoTinyS = 3;

template <typename T, class S0, class S1>
__global__ void __launch_bounds__((DwBody<T, S0>::NT > DwBody<T, S1>::NT ? DwBody<T, S0>::NT : DwBody<T, S1>::NT), 4)
dwconv7_ln_two_kernel(const DwGroupArgs<T> a0, const DwGroupArgs<T> a1, const int grid0, const float* __restrict__ wdw,
                      const float* __restrict__ bdw, const float* __restrict__ lnw, const float* __restrict__ lnb, float eps) {
  typedef DwBody<T, S0> B0;
  typedef DwBody<T, S1> B1;
  constexpr int NT = B0::NT > B1::NT ? B0::NT : B1::NT;
  static_assert(B0::NT % 64 == 0 && B1::NT % 64 == 0, "whole waves leave");
  extern __shared__ __attribute__((aligned(16))) unsigned char dw2_lds[];
  const int bx = blockIdx.x;
  // Whole waves leave (the test is on the wave's first lane: a scalar branch), and group 1's workgroups end their program
  // behind its body: were the two bodies to meet in a common exit block, the thread index would stay live across both
  // and cost each a spilled register.
  const int t0 = __builtin_amdgcn_readfirstlane((int)threadIdx.x);
  if (bx >= grid0) {
    if (B1::NT == NT || t0 < B1::NT) B1::run(dw2_lds, bx - grid0, (int)gridDim.x - grid0, a1, wdw, bdw, lnw, lnb, eps);
    __builtin_amdgcn_endpgm();
  }
  if (B0::NT == NT || t0 < B0::NT) B0::run(dw2_lds, bx, grid0, a0, wdw, bdw, lnw, lnb, eps);
}

// f(p0, S0, p1, S1) for a pair the table covers, otherwise g()
template <class S0, class S1, class F, class G> int dw_two_dispatch(const DwPlan& p0, const DwPlan& p1, F& f, G& g) {
  if constexpr (dw_two_roll_pair<S0, S1>()) {
    return f(p0, S0{}, p1, S1{});
  } else if constexpr (dw_two_tiny_pair<S0>() && S1::kind == DwKind::Tiny) {
    return p1.n == kDwTwoTinyS ? f(p0, S0{}, p1, DwShape<DwKind::Tiny, 768, kDwTwoTinyS>{}) : g();
  } else {
    return g();
  }
}

// plans both groups (x / y 16-byte `aligned` or not, per group; plan0 / plan1: their plan_nimg) and calls f or g as
// dw_two_dispatch
template <typename T, class F, class G>
int dw_select2(int nimg0, int H0, int W0, bool al0, int nimg1, int H1, int W1, bool al1, int C, F&& f, G&& g, int plan0 = 0,
               int plan1 = 0) {
  return dw_select<T>(nimg0, H0, W0, C, al0, [&](const DwPlan& p0, auto sh0) -> int {
    return dw_select<T>(nimg1, H1, W1, C, al1, [&](const DwPlan& p1, auto sh1) -> int {
      return dw_two_dispatch<decltype(sh0), decltype(sh1)>(p0, p1, f, g);
    }, plan1);
  }, plan0);
}

template <typename T> bool dw_two_merged(int nimg0, int H0, int W0, int nimg1, int H1, int W1, int C, bool aligned) {
  return dw_select2<T>(nimg0, H0, W0, aligned, nimg1, H1, W1, aligned, C,
                       [](const DwPlan&, auto, const DwPlan&, auto) { return 1; }, [] { return 0; }) == 1;
}

template <typename T>
int launch_dwconv7_ln2(const T* x0, T* y0, int nimg0, int H0, int W0, const T* x1, T* y1, int nimg1, int H1, int W1,
                       const float* wdw, const float* bdw, const float* lnw, const float* lnb, int C, float eps,
                       hipStream_t s, int plan0, int plan1) {
  auto al = [](const T* x, const T* y) { return ((reinterpret_cast<uintptr_t>(x) | reinterpret_cast<uintptr_t>(y)) & 15u) == 0; };
  return dw_select2<T>(
      nimg0, H0, W0, al(x0, y0), nimg1, H1, W1, al(x1, y1), C,
      [&](const DwPlan& p0, auto sh0, const DwPlan& p1, auto sh1) -> int {
        typedef DwBody<T, decltype(sh0)> B0;
        typedef DwBody<T, decltype(sh1)> B1;
        DwPlan p = p0;
        p.grid = p0.grid + p1.grid;
        p.block = std::max(B0::NT, B1::NT);
        p.lds = std::max(B0::lds, B1::lds);
        const DwGroupArgs<T> a0{x0, y0, H0, p0.band_rows, p0.band_rows ? cdiv(H0, p0.band_rows) : 0};
        const DwGroupArgs<T> a1{x1, y1, H1, p1.band_rows, p1.band_rows ? cdiv(H1, p1.band_rows) : 0};
        return dw_launch(p, dwconv7_ln_two_kernel<T, decltype(sh0), decltype(sh1)>, s, a0, a1, p0.grid, wdw, bdw, lnw, lnb,
                         eps);
      },
      [&]() -> int {
        GCV_TRY(launch_dwconv7_ln<T>(x0, wdw, bdw, lnw, lnb, y0, nimg0, H0, W0, C, eps, s, plan0));
        return launch_dwconv7_ln<T>(x1, wdw, bdw, lnw, lnb, y1, nimg1, H1, W1, C, eps, s, plan1);
      }, plan0, plan1);
}

#define GCV_INSTANTIATE_DW(T)                                                                                        \
  template int dw_plan<T>(DwPlan&, int, int, int, int, bool);                                                        \
  template int launch_dwconv7_ln<T>(const T*, const float*, const float*, const float*, const float*, T*, int, int,   \
                                    int, int, float, hipStream_t, int);                                              \
  template bool dw_two_merged<T>(int, int, int, int, int, int, int, bool);                                           \
  template int launch_dwconv7_ln2<T>(const T*, T*, int, int, int, const T*, T*, int, int, int, const float*,         \
                                     const float*, const float*, const float*, int, float, hipStream_t, int, int);

}  // namespace gcv
