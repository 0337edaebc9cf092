// The ConvNeXt block MLP, out = resid + gamma * (fc2 . GELU(fc1 . x + b1) + b2) (timm ConvNeXtBlock: mlp.fc1 -> GELU ->
// mlp.fc2 -> * gamma -> + shortcut), chosen in one place: mlp_kind picks a block's kernels, pack_cnx_mlp packs its weights
// for them, launch_cnx_mlp launches them and lnp_plan decides whether the stage boundary's LayerNorm-patchify runs in the
// epilogue.  The network (net_impl.h) and the kernel test entry (api.hip, gcv_k_fused_mlp*) both go through these.
#pragma once
#include "fused_mlp.h"
#include "gemm.h"
#include "mlp_pair.h"
#include "xs_mlp.h"

namespace gcv {

enum class MlpKind {
  Gemm,      // fp32, or 16-bit at C = 768: two tile GEMMs through the (M, 4C) hidden tensor
  Fused96,   // 16-bit, C = 96: fused_mlp_res_kernel when fused_mlp_res_applies(C, M), else fused_mlp_kernel<T, 96, 4>
  Xs192,     // 16-bit, C = 192: xs_mlp_kernel (xs_mlp.h)
  Pair384,   // 16-bit, C = 384: xs_pw1_kernel + pw2f_kernel through the fragment-major hidden tensor (mlp_pair.h)
};
static inline MlpKind mlp_kind(size_t tsize, int C) {
  if (tsize != 2) return MlpKind::Gemm;
  if (C == 96) return MlpKind::Fused96;
  if (C == 192) return MlpKind::Xs192;
  if (C == 384) return MlpKind::Pair384;
  return MlpKind::Gemm;
}

// one block's MLP weights: fp32 vectors, fc1 / fc2 in T ((N, K) row-major, nn.Linear layout) and what its kind packs
template <typename T> struct CnxMlpW {
  MlpKind kind = MlpKind::Gemm;
  const T* w1 = nullptr;           // fc1 (4C, C)
  const T* w2 = nullptr;           // fc2 (C, 4C): Gemm; Xs192 packs from it when it is set
  const float *b1 = nullptr, *b2 = nullptr, *gamma = nullptr;
  T* w2c = nullptr;                // Fused96: fc2 in kMlpHC-wide hidden chunks (pack_w2_chunks)
  T* wp = nullptr;                 // Xs192: fc1 | fc2 records (pack_xs_mlp)
  T *w1f = nullptr, *w2f = nullptr;   // Pair384: fc1 and gamma * fc2 in MFMA-fragment order
};

// Packs w's weights for w.kind (kind, w1, gamma set).  fc2 comes from w2_f32, fc2 in fp32 on the device, for the kinds that
// round it to T themselves (Fused96; Pair384, which folds gamma in), and for Xs192 when w.w2 is null.  alloc(bytes) returns
// device memory that lives as long as w, or null.  Enqueued on s: the caller synchronises before it frees w2_f32.
static inline bool mlp_packs_from_f32(MlpKind k) { return k == MlpKind::Fused96 || k == MlpKind::Pair384; }
template <typename T, class Alloc>
int pack_cnx_mlp(CnxMlpW<T>& w, int C, const float* w2_f32, Alloc&& alloc, hipStream_t s) {
  if constexpr (sizeof(T) == 2) {
    GCV_REQUIRE(w.w1 && (w.w2 || w2_f32) && (w2_f32 || !mlp_packs_from_f32(w.kind)), "MLP packing: fc1 / fc2 sources");
    const size_t wbytes = (size_t)4 * C * C * sizeof(T);
    switch (w.kind) {
      case MlpKind::Gemm: return 0;
      case MlpKind::Fused96:
        w.w2c = (T*)alloc(wbytes);
        if (!w.w2c) { set_error("hipMalloc failed for packed fc2"); return -5; }
        return launch_pack_w2_chunks<T>(w2_f32, w.w2c, C, s);
      case MlpKind::Xs192:
        w.wp = (T*)alloc(xs_mlp_packed_elems(C) * sizeof(T));
        if (!w.wp) { set_error("hipMalloc failed for the packed fc1 | fc2 records"); return -5; }
        if (w.w2) return launch_pack_xs_mlp<T, T>(w.w1, w.w2, w.wp, C, s);
        return launch_pack_xs_mlp<T, float>(w.w1, w2_f32, w.wp, C, s);
      case MlpKind::Pair384:
        w.w1f = (T*)alloc(wbytes);
        w.w2f = (T*)alloc(wbytes);
        if (!w.w1f || !w.w2f) { set_error("hipMalloc failed for the fragment-major fc1 / fc2"); return -5; }
        GCV_TRY((launch_pack_w1_frag<T, T>(w.w1, w.w1f, C, s)));
        // the layer scale is folded into the packed fc2, from the fp32 source so that gamma * W2 is rounded to T once
        return launch_pack_w2_frag<T, float>(w2_f32, w.gamma, w.w2f, C, s);
    }
  }
  return 0;
}

// The stage boundary's LayerNorm2d + 2x2 space-to-depth in the epilogue of the stage's last MLP (LnpArgs, mlp_parts.h): `out`
// then receives the patch rows (M/4, 4C) of the down-sampling GEMM and the (M, C) residual stream is not written.
// Whether kind has the epilogue at M tokens (C = 96: the LDS-resident kernel only):
static inline bool lnp_supported(MlpKind kind, int C, int64_t M) {
  return kind == MlpKind::Xs192 || (kind == MlpKind::Fused96 && fused_mlp_res_applies(C, M));
}
// Fills l for nseg (<= 4) token-contiguous segments of n[s] images with h[s] x wd[s] maps, and returns whether the
// epilogue fuses: lnp_supported, and every map even (an odd map drops its last row / column: the separate kernel does that).
static inline bool lnp_plan(LnpArgs& l, MlpKind kind, int C, int64_t M, int nseg, const int* n, const int* h,
                            const int* wd) {
  bool even = true;
  int64_t t = 0, o = 0;
  l.nseg = nseg;
  for (int s = 0; s < nseg; ++s) {
    l.tok0[s] = (int)t; l.hw[s] = h[s] * wd[s]; l.wd[s] = wd[s]; l.out0[s] = (int)o;
    t += (int64_t)n[s] * h[s] * wd[s];
    o += (int64_t)n[s] * (h[s] / 2) * (wd[s] / 2);
    even = even && h[s] % 2 == 0 && wd[s] % 2 == 0;
  }
  return even && lnp_supported(kind, C, M);
}

// What launch_cnx_mlp launches at M tokens, from the launchers' own geometry rules (gcv_mlp_plan; no HIP call).
// v by kind (include/genconvit_hip.h): Fused96 {LDS-resident kernel?, workgroups, wave tiles, most tiles per wave},
// Xs192 {passes, workgroups, most passes per workgroup}, Pair384 {pw1 tiles, ns, chunks per workgroup, pw2 BN, D, TB, grid}
struct MlpPlan {
  MlpKind kind = MlpKind::Gemm;
  int v[7] = {0, 0, 0, 0, 0, 0, 0};
};
static inline int mlp_plan(MlpPlan& p, size_t tsize, int C, int M, int wg_cap) {
  GCV_REQUIRE(M > 0 && wg_cap >= 1 && wg_cap <= kMlpWgCap, "MLP plan: M > 0, workgroup cap in [1, 256]");
  p = MlpPlan{};
  p.kind = mlp_kind(tsize, C);
  switch (p.kind) {
    case MlpKind::Gemm: break;
    case MlpKind::Fused96: {
      const int tiles = fused_mlp_wave_tiles(M);
      if (fused_mlp_res_applies(C, M)) {
        const int nwg = mlp_persistent_wgs(cdiv(tiles, kMlpResWaves), wg_cap);
        p.v[0] = 1; p.v[1] = nwg; p.v[2] = tiles; p.v[3] = cdiv(tiles, nwg * kMlpResWaves);
      } else {
        p.v[1] = fused_mlp_tile_wgs(M); p.v[2] = tiles; p.v[3] = 1;
      }
      break;
    }
    case MlpKind::Xs192: {
      const int npass = xs_mlp_passes(M), nwg = mlp_persistent_wgs(npass, wg_cap);
      p.v[0] = npass; p.v[1] = nwg; p.v[2] = cdiv(npass, nwg);
      break;
    }
    case MlpKind::Pair384: {
      const int nkc = 4 * C / 32, ntile = xs_pw1_tiles(M), ns = xs_pw1_pick_split(ntile, nkc);
      const Pw2fTile t = pw2f_pick(M, C);
      p.v[0] = ntile; p.v[1] = ns; p.v[2] = nkc / ns; p.v[3] = t.BN; p.v[4] = t.D; p.v[5] = t.TB; p.v[6] = t.grid;
      break;
    }
  }
  return 0;
}

// Launches the MLP of w.kind over M tokens of x.  hidden: the (M, 4C) tensor of Gemm, the fragment-major one of Pair384
// (mlp_pair_hidden_bytes).  lnp (lnp_plan returned true): the LN-patchify epilogue, into `out`.  Launches go through
// r.run(tag, flops, bytes, f) and r.gemm(tag, GemmArgs, a_mode, epi) on stream s (NetImpl: tagged and profiled).
// wg_cap: the persistent kernels' workgroup limit; below kMlpWgCap from the kernel test entries only (mlp_parts.h).
template <typename T, class R>
int launch_cnx_mlp(R& r, const CnxMlpW<T>& w, int C, const T* x, const T* resid, T* out, T* hidden, int M,
                   const LnpArgs* lnp, hipStream_t s, int wg_cap = kMlpWgCap) {
  GCV_REQUIRE(!lnp || lnp_supported(w.kind, C, M), "LN-patchify epilogue of an MLP kind without one");
  if constexpr (sizeof(T) == 2) {
    const double fused_flops = 16.0 * M * C * (double)C, fused_bytes = 3.0 * sizeof(T) * (double)M * C + 16.0 * C * C;
    switch (w.kind) {
      case MlpKind::Gemm: break;
      case MlpKind::Fused96: {
        MlpArgs a{x, w.w1, w.b1, w.w2c, w.b2, w.gamma, resid, out, M};
        if (lnp) a.lnp = *lnp;
        return r.run("cnx.fused_mlp", fused_flops, fused_bytes, [&] { return launch_fused_mlp<T>(a, C, s, wg_cap); });
      }
      case MlpKind::Xs192: {
        XsMlpArgs a{x, w.wp, w.b1, w.b2, w.gamma, resid, out, M};
        if (lnp) a.lnp = *lnp;
        return r.run("cnx.fused_mlp", fused_flops, fused_bytes, [&] { return launch_xs_mlp<T>(a, C, s, wg_cap); });
      }
      case MlpKind::Pair384: {
        MlpPairArgs a{x, w.w1f, w.b1, w.w2f, w.b2, w.gamma, resid, out, hidden, M};
        GCV_TRY(r.run("cnx.pw1_gelu", 8.0 * M * C * (double)C, sizeof(T) * (5.0 * M * C + 4.0 * C * C),
                      [&] { return launch_xs_pw1<T>(a, C, s); }));
        return r.run("cnx.pw2_scale_res", 8.0 * M * C * (double)C, sizeof(T) * (6.0 * M * C + 4.0 * C * C),
                     [&] { return launch_pw2f<T>(a, C, s); });
      }
    }
  }
  GemmArgs g1{};
  g1.A = x; g1.lda = C; g1.Wt = w.w1; g1.C = hidden; g1.ldc = 4 * C; g1.bias = w.b1;
  g1.M = M; g1.N = 4 * C; g1.K = C; g1.act = ACT_GELU; g1.splitk = 1;
  GCV_TRY(r.gemm("cnx.pw1_gelu", g1, A_PLAIN, EPI_BIAS_ACT));
  GemmArgs g2{};
  g2.A = hidden; g2.lda = 4 * C; g2.Wt = w.w2; g2.C = out; g2.ldc = C; g2.bias = w.b2; g2.gamma = w.gamma;
  g2.resid = resid; g2.M = M; g2.N = C; g2.K = 4 * C; g2.act = ACT_NONE; g2.splitk = 1;
  return r.gemm("cnx.pw2_scale_res", g2, A_PLAIN, EPI_RESID);
}

}  // namespace gcv
