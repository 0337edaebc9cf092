// launchers + weight packer of the C = 96 fused MLP kernels (included by fused_mlp_{f16,bf16}.hip)
#pragma once
#include "fused_mlp.h"
#include "fused_mlp_res.h"

namespace gcv {

// W2 (C, 4C) fp32 row-major -> [4C/HC][C][HC] in T; inside every 16 hidden indices bits 2 and 3 are
// swapped so that a lane's GEMM2 A-operand fragment (k = 16kk + 8(j>>2) + 4h + (j&3)) is one 16-byte chunk.
template <typename T>
__global__ void __launch_bounds__(256) pack_w2_chunks_kernel(const float* __restrict__ w2, T* __restrict__ out, int C,
                                                             int HC) {
  const int64_t total = (int64_t)C * 4 * C;
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= total) return;
  const int p = (int)(i % HC);
  const int64_t t = i / HC;
  const int o = (int)(t % C);
  const int ch = (int)(t / C);
  const int kk = p >> 4, h = (p >> 3) & 1, jj = p & 7;
  const int hid = 16 * kk + 8 * (jj >> 2) + 4 * h + (jj & 3);
  out[i] = from_f<T>(w2[(int64_t)o * 4 * C + ch * HC + hid]);
}

template <typename T> int launch_pack_w2_chunks(const float* w2_dev, T* out, int C, hipStream_t s) {
  constexpr int HC = kMlpHC;
  GCV_REQUIRE((4 * C) % HC == 0, "hidden width must be a multiple of the chunk");
  const int64_t total = (int64_t)C * 4 * C;
  hipLaunchKernelGGL((pack_w2_chunks_kernel<T>), dim3((unsigned)cdiv64(total, 256)), dim3(256), 0, s, w2_dev, out, C, HC);
  GCV_CHECK_HIP(hipGetLastError());
  return 0;
}

template <typename T> int launch_fused_mlp_res(const MlpArgs& a, hipStream_t s, int wg_cap) {
  constexpr int SMEM = MlpResSmem::bytes;
  GCV_ENSURE_LDS((fused_mlp_res_kernel<T>), SMEM);
  constexpr int nw = kMlpResWaves;
  const int nwg = mlp_persistent_wgs(cdiv(fused_mlp_wave_tiles(a.M), nw), wg_cap);    // one persistent workgroup per CU
  if (a.lnp.nseg > 0) {                                    // last block of the stage: LayerNorm2d + space-to-depth epilogue
    GCV_REQUIRE(a.lnp.w && a.lnp.b && a.lnp.nseg <= 4, "fused MLP: LN-patchify epilogue arguments");
    GCV_ENSURE_LDS((fused_mlp_res_kernel<T, true>), SMEM);
    hipLaunchKernelGGL((fused_mlp_res_kernel<T, true>), dim3(nwg), dim3(64 * nw), SMEM, s, a);
  } else {
    hipLaunchKernelGGL((fused_mlp_res_kernel<T>), dim3(nwg), dim3(64 * nw), SMEM, s, a);
  }
  GCV_CHECK_HIP(hipGetLastError());
  return 0;
}

template <typename T> int launch_fused_mlp(const MlpArgs& a, int C, hipStream_t s, int wg_cap) {
  GCV_REQUIRE(a.M > 0 && a.X && a.W1 && a.W2c && a.b1 && a.b2 && a.gamma && a.resid && a.out, "fused MLP: null argument");
  GCV_REQUIRE(wg_cap >= 1 && wg_cap <= kMlpWgCap, "fused MLP: workgroup cap in [1, 256]");
  // with enough tokens to give every wave of the chip several tiles: weights resident in LDS, no barriers
  if (fused_mlp_res_applies(C, a.M)) return launch_fused_mlp_res<T>(a, s, wg_cap);
  GCV_REQUIRE(a.lnp.nseg == 0, "fused MLP: the LN-patchify epilogue exists in the LDS-resident kernel only");
  GCV_REQUIRE(C == MlpSmem::C, "fused MLP kernels of this file: C = 96");
  constexpr int SMEM = MlpSmem::bytes, NW = MlpSmem::NW;
  GCV_ENSURE_LDS((fused_mlp_kernel<T>), SMEM);
  static_assert(NW == kMlpTileWaves, "fused_mlp_tile_wgs");
  hipLaunchKernelGGL((fused_mlp_kernel<T>), dim3(fused_mlp_tile_wgs(a.M)), dim3(NW * 64), SMEM, s, a);
  GCV_CHECK_HIP(hipGetLastError());
  return 0;
}

}  // namespace gcv
