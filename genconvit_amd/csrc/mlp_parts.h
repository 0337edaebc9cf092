// What the hand-written 16-bit ConvNeXt MLP kernels have in common (fused_mlp.h, fused_mlp_res.h, xs_mlp.h, mlp_pair.h; the
// wait also serves the ring of gemm_glds.h).  These kernels sit at their register limits, so a piece lives here only if
// every translation unit that uses it compiles to the device code it had with the piece written out in place; what did
// not pass that test stays in its kernel with a comment that says so.
#pragma once
#include "gemm.h"

namespace gcv {

template <typename T> using vec4 = T __attribute__((ext_vector_type(4)));

// DMAs (and loads) down to N outstanding, then the workgroup barrier: one asm statement, so that no LDS access can be
// scheduled between the wait and the barrier
#define GCV_WAIT_BARRIER(N) asm volatile("s_waitcnt vmcnt(%0)\n\ts_barrier" ::"n"(N) : "memory")

// A token row's 16-byte piece <-> the two 8-byte halves of the MFMA accumulator layout.  Lane (token lr, half lh) of an
// accumulator holds channels 8q + 4lh .. + 3 of every group q; of a (q, q + 1) pair of groups, a row's 16-byte piece has
// channels 8q .. 8q + 7 in lanes 0-31 and 8q + 8 .. 8q + 15 in lanes 32-63.  One v_permlane32_swap per dword converts
// (lanes 32-63 of the first operand <-> lanes 0-31 of the second); it is its own inverse.
template <typename T> __device__ __forceinline__ void piece_to_halves(const u32x4 pc, vec4<T> (&h)[2]) {
  const auto x = __builtin_amdgcn_permlane32_swap(pc[0], pc[2], false, false);
  const auto y = __builtin_amdgcn_permlane32_swap(pc[1], pc[3], false, false);
  h[0] = __builtin_bit_cast(vec4<T>, uint2{x[0], y[0]});
  h[1] = __builtin_bit_cast(vec4<T>, uint2{x[1], y[1]});
}
__device__ __forceinline__ u32x4 halves_to_piece(const uint2 (&h)[2]) {
  const auto x = __builtin_amdgcn_permlane32_swap(h[0].x, h[1].x, false, false);
  const auto y = __builtin_amdgcn_permlane32_swap(h[0].y, h[1].y, false, false);
  return u32x4{x[0], y[0], x[1], y[1]};
}

// The persistent kernels (fused_mlp_res_kernel, xs_mlp_kernel) launch at most this many workgroups, one per CU.  The kernel
// test entries gcv_k_fused_mlp*_planned pass a lower cap, so that a few thousand tokens run the passes per workgroup of a
// large batch; the networks never do.
constexpr int kMlpWgCap = 256;
// workgroups of a persistent kernel with `units` workgroup-sized pieces of work
static inline int mlp_persistent_wgs(int units, int wg_cap) { return units < wg_cap ? units : wg_cap; }

// Optional epilogue of the LAST block of a stage (fused_mlp_res_kernel, xs_mlp_kernel): the stage boundary's LayerNorm2d +
// 2x2 space-to-depth (timm ConvNeXt `downsample`: LayerNorm2d -> Conv2d(k=2, s=2)) applied to the output rows,
// which nothing else needs: `out` is then the patchified (M/4, 4C) operand of the down-sampling GEMM and the (M, C) residual
// stream is not written at all.  Tokens [tok0[s], tok0[s+1]) are images of hw[s] = H*W pixels, W = wd[s]; their patch rows
// start at out0[s].  nseg == 0: no such epilogue.  (Part of the kernel arguments: the field order is their layout.)
struct LnpArgs {
  const float* w = nullptr;   // LayerNorm2d weight | bias (C)
  const float* b = nullptr;
  float eps = 0.0f;
  int nseg = 0;
  int tok0[4] = {0, 0, 0, 0};
  int hw[4] = {1, 1, 1, 1};
  int wd[4] = {1, 1, 1, 1};
  int out0[4] = {0, 0, 0, 0};
};

// LayerNorm statistics of a token row whose C channels are the acc2 of lanes l and l + 32, from the lane's sums s1 / s2:
// rstd and -mean * rstd.  One pass cancels once the channels share an offset (common.h, kLnRecentre): the squares of the
// centred values then stand in for E[x^2] - mean^2.  BRANCH: they are summed only where needed (lanes l and l + 32 hold the
// same mean and s2 and decide alike); else always, and selected.
template <int C, bool BRANCH>
__device__ __forceinline__ void lnp_stats(const f32x16 (&acc2)[C / 32], float s1, float s2, const float eps, float& rstd,
                                          float& nmr) {
  s1 += __shfl_xor(s1, 32);                                // the other half of the row's channels lives in lane ^ 32
  s2 += __shfl_xor(s2, 32);
  const float mean = s1 * (1.0f / C);
  auto centred = [&]() {
    float sc = 0.0f;
#pragma unroll
    for (int o = 0; o < C / 32; ++o)
#pragma unroll
      for (int e = 0; e < 16; ++e) sc = fmaf(acc2[o][e] - mean, acc2[o][e] - mean, sc);
    return sc + __shfl_xor(sc, 32);
  };
  float var;
  if constexpr (BRANCH) {
    var = fmaf(-mean, mean, s2 * (1.0f / C));
    if (var < s2 * (kLnRecentre / C)) var = centred() * (1.0f / C);
  } else {
    const float sc = centred();
    const float var1 = fmaf(-mean, mean, s2 * (1.0f / C));
    var = var1 < s2 * (kLnRecentre / C) ? sc * (1.0f / C) : var1;
  }
  rstd = __builtin_amdgcn_rsqf(fmaxf(var, 0.0f) + eps);
  nmr = -mean * rstd;
}

}  // namespace gcv
