// The GEMM family (every network, the explain backward and Swin launch through it): gemm_select validates a launch and picks
// its kernel, tile and grid in one place, launch_gemm launches from that plan and gemm_plan returns the plan without a HIP
// call.  Included by gemm_{f32,f16,bf16}.hip.
#pragma once
#include <algorithm>

#include "conv_direct.h"
#include "gemm.h"
#include "gemm_glds.h"

namespace gcv {

static inline bool aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15u) == 0; }

// default LDS row: 64 B for fp32 (16 k), 128 B for 16-bit (64 k)
template <typename T> struct DefBKB { static constexpr int v = sizeof(T) == 4 ? 64 : 128; };

// The three kinds of kernel.  plan<T, EPI>(g): tile fields, grid, threads and dynamic LDS bytes of the launch g;
// kernel<T, AMODE, EPI, ACT>(): the instantiation.
template <int BM, int BN, int WM, int WN, int BKB> struct TileShape {
  static constexpr GemmKind kind = GemmKind::Tile;
  template <typename T, int EPI> static GemmPlan plan(const GemmArgs& g) {
    return {kind, BM, BN, WM, WN, BKB, cdiv(g.M, BM) * cdiv(g.N, BN), EPI == EPI_SPLITK ? g.splitk : 1, 256,
            GemmSmem<T, BM, BN, BKB, EPI>::bytes};
  }
  template <typename T, int AMODE, int EPI, int ACT> static constexpr auto kernel() {
    return gemm_kernel<T, BM, BN, WM, WN, BKB, AMODE, EPI, ACT>;
  }
};
template <int BKB> struct GldsShape {
  static constexpr GemmKind kind = GemmKind::Glds;
  template <typename T, int EPI> static GemmPlan plan(const GemmArgs& g) {
    return {kind, kGldsBM, kGldsBN, kGldsBM / 2, kGldsBN / 2, BKB, cdiv(g.M, kGldsBM) * (g.N / kGldsBN), 1, 256,
            GldsSmem<T, BKB>::bytes};
  }
  template <typename T, int AMODE, int EPI, int ACT> static constexpr auto kernel() { return gemm_glds_kernel<T, EPI, ACT, BKB>; }
};
// workgroups of four waves; a wave takes at least two 32-row pixel blocks where there are that many (the second block's loads
// run under the first block's MFMAs), and at most kConvDirectMaxWg workgroups are launched
template <int CIN, int STRIDE> struct DirectShape {
  static constexpr GemmKind kind = GemmKind::Direct;
  template <typename T, int EPI> static GemmPlan plan(const GemmArgs& g) {
    return {kind, CIN, STRIDE, 0, 0, 0, std::min(kConvDirectMaxWg, cdiv(cdiv(g.M, 32) * (g.N / 32), 8)), 1, 256, 0};
  }
  template <typename T, int AMODE, int EPI, int ACT> static constexpr auto kernel() { return conv3_direct_kernel<T, CIN, STRIDE>; }
};

// an (a_mode, epilogue) pair of gemm_select and the activations its kernels are built for
template <int AMODE, int EPI, int... ACTS> struct Route {};
typedef Route<A_PLAIN, EPI_BIAS_ACT, ACT_NONE, ACT_RELU, ACT_GELU, ACT_LEAKY> Linear;
typedef Route<A_PLAIN, EPI_BIAS_ACT, ACT_NONE, ACT_GELU> LinearDma;
typedef Route<A_PLAIN, EPI_RESID, ACT_NONE> Resid;
typedef Route<A_PLAIN, EPI_CONVT, ACT_RELU, ACT_LEAKY> ConvT;
typedef Route<A_PLAIN, EPI_SPLITK, ACT_NONE> SplitK;
typedef Route<A_IM2COL3_POOL, EPI_POOL4, ACT_RELU> ConvPool;
typedef Route<A_IM2COL3_S2, EPI_BIAS_ACT, ACT_LEAKY> ConvS2;

// what gemm_select hands to f beside the plan: the kernel of shape S on a route, with activation ACT
template <typename T, class S, int AMODE, int EPI, int ACT> struct GemmPick {
  static constexpr GemmKind kind = S::kind;
  static constexpr auto kernel() { return S::template kernel<T, AMODE, EPI, ACT>(); }
};
// the activation fan-out: plans shape S for g and calls f with the instantiation of the route's activation `act`
template <typename T, int AMODE, int EPI, int... ACTS, class S, class F>
int gemm_pick(Route<AMODE, EPI, ACTS...>, S, const GemmArgs& g, int act, F& f) {
  const GemmPlan p = S::template plan<T, EPI>(g);
  int rc = -2;
  if (!((act == ACTS && ((rc = f(p, GemmPick<T, S, AMODE, EPI, ACTS>{})), true)) || ...)) set_error("bad activation code");
  return rc;
}

// The launch g of (a_mode, epi) in storage dtype T: validates it, picks the kernel (DESIGN.md has the table), fills a
// GemmPlan and returns f(plan, GemmPick), or sets the launcher's error.  Every (kind, shape, route) named here has a GPU
// parity case (tests/gemmcases.py; tests/test_host_cpu.py checks the set and pins the choice against tests/golden/gemm_plan.json).
template <typename T, class F> int gemm_select(const GemmArgs& g, int a_mode, int epi, F&& f) {
  constexpr int EPC = DT<T>::EPC;
  constexpr int B = DefBKB<T>::v;
  constexpr int BK = B / 16 * EPC;
  constexpr bool h16 = sizeof(T) == 2;
  GCV_REQUIRE(g.M > 0 && g.N > 0 && g.K > 0, "empty GEMM");
  GCV_REQUIRE(g.K % EPC == 0, "K must be a multiple of the 16-byte chunk");
  GCV_REQUIRE(g.N % 4 == 0, "N must be a multiple of 4");
  GCV_REQUIRE(aligned16(g.A) && aligned16(g.Wt), "A/Wt must be 16-byte aligned");
  if (epi != EPI_SPLITK) {
    GCV_REQUIRE(g.C && (reinterpret_cast<uintptr_t>(g.C) % (4 * sizeof(T))) == 0, "C must be aligned to 4 elements");
    GCV_REQUIRE(epi == EPI_CONVT || (g.ldc % 4 == 0 && g.ldc >= g.N), "ldc must be a multiple of 4 and >= N");
    GCV_REQUIRE(!g.bias || aligned16(g.bias), "bias must be 16-byte aligned");
  }
  if (a_mode == A_PLAIN) {
    GCV_REQUIRE(g.lda % EPC == 0 && g.lda >= g.K, "lda must be a chunk multiple >= K");
  } else {
    GCV_REQUIRE((1 << g.cin_log2) % EPC == 0 && g.K == 9 * (1 << g.cin_log2), "im2col: K = 9*Cin, Cin chunk-aligned");
    GCV_REQUIRE((g.H % 2) == 0 && (g.W % 2) == 0, "im2col modes need even H, W");
  }
  if (epi == EPI_SPLITK) {
    GCV_REQUIRE(g.splitk >= 1 && g.k_per_split % BK == 0 && (int64_t)g.k_per_split * g.splitk >= g.K && g.partial &&
                aligned16(g.partial), "bad split-K plan");
  }
  if (epi == EPI_RESID) GCV_REQUIRE(g.gamma && g.resid && aligned16(g.gamma), "EPI_RESID needs gamma and resid");
  if (epi == EPI_POOL4) GCV_REQUIRE(g.M % 4 == 0, "EPI_POOL4 needs M % 4 == 0");
  if (epi == EPI_CONVT) GCV_REQUIRE(g.N == 4 << g.cout_log2 && g.cout_log2 >= 2 && g.M % (g.H * g.W) == 0, "EPI_CONVT shape");

  const int act = epi == EPI_SPLITK ? ACT_NONE : g.act;      // a split-K slab has no activation: g.act is not read
  auto go = [&](auto route, auto shape) { return gemm_pick<T>(route, shape, g, act, f); };
  // 16-bit GEMMs whose K leaves a tail of <= 32 use 64-byte LDS rows (K tile 32) instead of padding a 64-k tile
  const bool short_k = h16 && (g.K % 64) != 0 && (g.K % 64) <= 32;
  // gemm_glds_kernel (gemm_glds.h), 16-bit storage: whole 128 x 192 tiles along N, no K tail, at least two M tiles, 16-byte
  // stores (what the checks above leave open of them; EPI_RESID also reads resid 8 bytes at a time)
  const bool dma = h16 && g.N % kGldsBN == 0 && g.K % 32 == 0 && g.M >= 256 && g.ldc % 8 == 0 &&
                   aligned16(g.C) && (epi != EPI_RESID || (reinterpret_cast<uintptr_t>(g.resid) & 7u) == 0);
  // ... on 128-byte LDS rows (K = 384: 6 stages, the 4-deep ring of 64-byte rows wins)
  const bool dma128 = g.K % 64 == 0 && g.K >= 512;

  if (a_mode == A_PLAIN && epi == EPI_BIAS_ACT) {
    if constexpr (h16)
      if (dma && (act == ACT_NONE || act == ACT_GELU))
        return dma128 ? go(LinearDma{}, GldsShape<128>{}) : go(LinearDma{}, GldsShape<64>{});
    // small problems (the classifier heads: M = frames <= 256, N = 500 / 1000): with 128-row tiles they are 4-16
    // workgroups on a 256-CU chip and take 20-50 us of pure latency; 32- / 64-row tiles spread the same work over 4x / 2x
    // as many CUs
    const int t128 = cdiv(g.M, 128) * cdiv(g.N, 128);
    if (g.M <= 32 || t128 < 48) return go(Linear{}, TileShape<32, 128, 32, 32, B>{});
    if (g.M <= 64 || t128 < 96) return go(Linear{}, TileShape<64, 128, 32, 64, B>{});
    if (g.N % 96 == 0 && short_k) return go(Linear{}, TileShape<128, 96, 32, 96, 64>{});
    if (g.N % 96 == 0) return go(Linear{}, TileShape<128, 96, 32, 96, B>{});
    return go(Linear{}, TileShape<128, 128, 64, 64, B>{});
  }
  if (a_mode == A_PLAIN && epi == EPI_RESID) {
    GCV_REQUIRE(g.act == ACT_NONE, "EPI_RESID has no activation");
    if constexpr (h16)
      if (dma) return dma128 ? go(Resid{}, GldsShape<128>{}) : go(Resid{}, GldsShape<64>{});
    if (g.N % 96 == 0) return go(Resid{}, TileShape<128, 96, 32, 96, B>{});
    return go(Resid{}, TileShape<128, 128, 64, 64, B>{});
  }
  if (a_mode == A_PLAIN && epi == EPI_CONVT) {
    GCV_REQUIRE(g.act == ACT_RELU || g.act == ACT_LEAKY, "EPI_CONVT is built for ReLU / LeakyReLU");
    if (g.N <= 64 && short_k) return go(ConvT{}, TileShape<128, 64, 32, 64, 64>{});
    if (g.N <= 64) return go(ConvT{}, TileShape<128, 64, 32, 64, B>{});
    return go(ConvT{}, TileShape<128, 128, 64, 64, B>{});
  }
  if (a_mode == A_PLAIN && epi == EPI_SPLITK) {
    if (g.M <= 32) return go(SplitK{}, TileShape<32, 128, 32, 32, B>{});
    if (g.M <= 64) return go(SplitK{}, TileShape<64, 128, 32, 64, B>{});
    return go(SplitK{}, TileShape<128, 128, 64, 64, B>{});
  }
  const bool pool = a_mode == A_IM2COL3_POOL && epi == EPI_POOL4;
  if (pool || (a_mode == A_IM2COL3_S2 && epi == EPI_BIAS_ACT)) {
    if (pool) GCV_REQUIRE(g.act == ACT_RELU, "conv3x3+pool is built for ReLU");
    else GCV_REQUIRE(g.act == ACT_LEAKY, "conv3x3 stride 2 is built for LeakyReLU");
    if constexpr (h16) {
      // conv3_direct_kernel (conv_direct.h), 16-bit storage, N = 32 / 64 with a bias: both MFMA operands straight from
      // memory.  It keeps 32-bit byte offsets into the input and 32-bit row numbers with a block of slack, and its stride-2
      // epilogue stores 16-byte pieces.  GCV_CONV_DIRECT says which (mode, Cin) are built
      const int cin = 1 << g.cin_log2;
      const bool fits = (int64_t)g.M * (pool ? 1 : 4) * cin * 2 < (int64_t(1) << 31) && g.M <= (1 << 30);
      if ((g.N == 32 || g.N == 64) && g.bias && fits && (pool || (aligned16(g.C) && g.ldc % 8 == 0))) {
        if constexpr (conv_direct_on(true, 16)) if (pool && cin == 16) return go(ConvPool{}, DirectShape<16, 1>{});
        if constexpr (conv_direct_on(true, 32)) if (pool && cin == 32) return go(ConvPool{}, DirectShape<32, 1>{});
        if constexpr (conv_direct_on(false, 16)) if (!pool && cin == 16) return go(ConvS2{}, DirectShape<16, 2>{});
        if constexpr (conv_direct_on(false, 32)) if (!pool && cin == 32) return go(ConvS2{}, DirectShape<32, 2>{});
      }
    }
    // K = 144 / 288 (16 / 32 input channels): 32-deep K tiles instead of a 64-deep one that is three quarters / half padding
    // (round 4, paired runs on one box: ed.enc 0.200 -> 0.171 ms, vae.enc 0.077 -> 0.068 ms per step)
    auto tiles = [&](auto route) {
      if (g.N <= 32 && short_k) return go(route, TileShape<128, 32, 32, 32, 64>{});
      if (g.N <= 64 && short_k) return go(route, TileShape<128, 64, 32, 64, 64>{});
      if (g.N <= 32) return go(route, TileShape<128, 32, 32, 32, B>{});
      if (g.N <= 64) return go(route, TileShape<128, 64, 32, 64, B>{});
      return go(route, TileShape<128, 128, 64, 64, B>{});
    };
    return pool ? tiles(ConvPool{}) : tiles(ConvS2{});
  }
  set_error("launch_gemm: unsupported (a_mode, epilogue) combination");
  return -3;
}

template <typename T> int gemm_plan(GemmPlan& p, const GemmArgs& g, int a_mode, int epi) {
  return gemm_select<T>(g, a_mode, epi, [&](const GemmPlan& q, auto) { p = q; return 0; });
}

template <typename T> int launch_gemm(const GemmArgs& g, int a_mode, int epi, hipStream_t s) {
  return gemm_select<T>(g, a_mode, epi, [&](const GemmPlan& p, auto pick) -> int {
    typedef decltype(pick) K;
    const dim3 grid(p.grid_x, p.grid_y), block(p.threads);
    if (K::kind == GemmKind::Glds || p.lds > 64 * 1024) GCV_ENSURE_LDS(K::kernel(), p.lds);
    if constexpr (K::kind == GemmKind::Direct) hipLaunchKernelGGL(K::kernel(), grid, block, p.lds, s, conv_direct_args(g));
    else hipLaunchKernelGGL(K::kernel(), grid, block, p.lds, s, g);
    GCV_CHECK_HIP(hipGetLastError());
    return 0;
  });
}

#define GCV_INSTANTIATE_GEMM(T)                                          \
  template int gemm_plan<T>(GemmPlan&, const GemmArgs&, int, int);       \
  template int launch_gemm<T>(const GemmArgs&, int, int, hipStream_t);

}  // namespace gcv
