// Stage-3 backward kernels of the layer-2 Grad-CAM (cam_bwd.h), instantiated for the three storage dtypes.
#include "cam_bwd.h"

namespace gcv {

// sum / max over the NW waves of a workgroup; `red` holds NW floats and is reused after the call's barrier pair
template <int NW> __device__ __forceinline__ float block_sum(float v, float* red) {
  v = wave_sum(v);
  __syncthreads();
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
  __syncthreads();
  float s = red[0];
#pragma unroll
  for (int i = 1; i < NW; ++i) s += red[i];
  return s;
}
template <int NW> __device__ __forceinline__ float block_max(float v, float* red) {
  v = wave_max(v);
  __syncthreads();
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
  __syncthreads();
  float s = red[0];
#pragma unroll
  for (int i = 1; i < NW; ++i) s = fmaxf(s, red[i]);
  return s;
}

// exact-erf GELU'(x) = Phi(x) + x phi(x)
__device__ __forceinline__ float gelu_grad(float x) {
  return 0.5f * (1.0f + erff(x * 0.70710678118654752440f)) + x * 0.39894228040143267794f * __expf(-0.5f * x * x);
}

// the exponent e with mx * 2^e in [0.5, 1) (0 for a zero or non-finite row), clamped so that 2^e and 2^-e are normal floats
__device__ __forceinline__ int row_exponent(float mx) {
  if (!(mx > 0.0f) || !(mx < 3.0e38f)) return 0;
  int e;
  (void)frexpf(mx, &e);
  return max(-120, min(120, -e));
}

// one workgroup per (frame, pass): the pooled row, its LayerNorm statistics and the LayerNorm backward as cam_kernel
// (cam.hip) forms them; the pooled row's gradient spreads evenly over the hw tokens
template <typename T, int C>
__global__ void __launch_bounds__(256) pool_ln_bwd_kernel(PoolLnBwdArgs p) {
  constexpr int NV = C / 256;
  __shared__ float red[4];
  const int b = blockIdx.x, pass = blockIdx.y, tid = threadIdx.x;
  const int hw = p.hw[pass];
  const T* A = (const T*)p.A[pass] + (int64_t)b * hw * C;
  float m[NV];
#pragma unroll
  for (int k = 0; k < NV; ++k) m[k] = 0.0f;
  for (int q = 0; q < hw; ++q) {
#pragma unroll
    for (int k = 0; k < NV; ++k) m[k] += to_f(A[(int64_t)q * C + tid + 256 * k]);
  }
  const float inv = 1.0f / (float)hw;
  float msum = 0.0f;
#pragma unroll
  for (int k = 0; k < NV; ++k) { m[k] *= inv; msum += m[k]; }
  const float mean = block_sum<4>(msum, red) / (float)C;
  float d2 = 0.0f;
#pragma unroll
  for (int k = 0; k < NV; ++k) { const float d = m[k] - mean; d2 = fmaf(d, d, d2); }
  const float rstd = 1.0f / sqrtf(block_sum<4>(d2, red) / (float)C + p.eps);
  const float* dp = p.dpool + ((int64_t)b * p.npass + pass) * C;
  float dy[NV], xh[NV], s1 = 0.0f, s2 = 0.0f;
#pragma unroll
  for (int k = 0; k < NV; ++k) {
    const int c = tid + 256 * k;
    dy[k] = dp[c] * p.lnw[c];
    xh[k] = (m[k] - mean) * rstd;
    s1 += dy[k];
    s2 = fmaf(dy[k], xh[k], s2);
  }
  const float mdy = block_sum<4>(s1, red) / (float)C;
  const float mdyx = block_sum<4>(s2, red) / (float)C;
  float* out = p.dA + ((int64_t)p.tok0[pass] + (int64_t)b * hw) * C;
#pragma unroll
  for (int k = 0; k < NV; ++k) {
    const float g = rstd * (dy[k] - mdy - xh[k] * mdyx) * inv;
    for (int q = 0; q < hw; ++q) out[(int64_t)q * C + tid + 256 * k] = g;
  }
}

// one workgroup per row of C = 256 NV values
template <typename T, int NV>
__global__ void __launch_bounds__(256) scale_rows_kernel(const float* __restrict__ g, const float* __restrict__ gamma,
                                                         T* __restrict__ out, float* __restrict__ inv) {
  constexpr int C = 256 * NV;
  __shared__ float red[4];
  const int tid = threadIdx.x;
  const int64_t row = blockIdx.x;
  float v[NV], mx = 0.0f;
#pragma unroll
  for (int k = 0; k < NV; ++k) {
    const int c = tid + 256 * k;
    v[k] = g[row * C + c] * (gamma ? gamma[c] : 1.0f);
    mx = fmaxf(mx, fabsf(v[k]));
  }
  const int e = row_exponent(block_max<4>(mx, red));
  const float sc = ldexpf(1.0f, e);
#pragma unroll
  for (int k = 0; k < NV; ++k) out[row * C + tid + 256 * k] = from_f<T>(v[k] * sc);
  if (tid == 0) inv[row] = ldexpf(1.0f, -e);
}

template <typename T, int NV>
__global__ void __launch_bounds__(256) gelu_bwd_kernel(const float* __restrict__ dh, const float* __restrict__ inv_in,
                                                       T* pre, float* __restrict__ inv_out) {
  constexpr int C = 256 * NV;
  __shared__ float red[4];
  const int tid = threadIdx.x;
  const int64_t row = blockIdx.x;
  const float s = inv_in[row];
  float v[NV], mx = 0.0f;
#pragma unroll
  for (int k = 0; k < NV; ++k) {
    const int64_t i = row * C + tid + 256 * k;
    v[k] = dh[i] * s * gelu_grad(to_f(pre[i]));
    mx = fmaxf(mx, fabsf(v[k]));
  }
  const int e = row_exponent(block_max<4>(mx, red));
  const float sc = ldexpf(1.0f, e);
#pragma unroll
  for (int k = 0; k < NV; ++k) pre[row * C + tid + 256 * k] = from_f<T>(v[k] * sc);
  if (tid == 0) inv_out[row] = ldexpf(1.0f, -e);
}

// one workgroup per token
template <typename T, int C>
__global__ void __launch_bounds__(256) dw_ln_bwd_kernel(DwLnBwdArgs p) {
  constexpr int NV = C / 256;
  __shared__ float red[4];
  const int tid = threadIdx.x, S = p.side, hw = S * S;
  const int64_t tok = blockIdx.x;
  const int img = (int)(tok / hw), q = (int)(tok - (int64_t)img * hw), y = q / S, x = q - y * S;
  const T* X = (const T*)p.x + (int64_t)img * hw * C;
  float acc[NV];
#pragma unroll
  for (int k = 0; k < NV; ++k) acc[k] = p.dw_b[tid + 256 * k];
  for (int ky = 0; ky < 7; ++ky) {
    const int ny = y + ky - 3;
    if (ny < 0 || ny >= S) continue;
    for (int kx = 0; kx < 7; ++kx) {
      const int nx = x + kx - 3;
      if (nx < 0 || nx >= S) continue;
#pragma unroll
      for (int k = 0; k < NV; ++k) {
        const int c = tid + 256 * k;
        acc[k] = fmaf(to_f(X[(int64_t)(ny * S + nx) * C + c]), p.dw_w[(ky * 7 + kx) * C + c], acc[k]);
      }
    }
  }
  float s0 = 0.0f;
#pragma unroll
  for (int k = 0; k < NV; ++k) s0 += acc[k];
  const float mean = block_sum<4>(s0, red) / (float)C;
  float d2 = 0.0f;
#pragma unroll
  for (int k = 0; k < NV; ++k) { acc[k] -= mean; d2 = fmaf(acc[k], acc[k], d2); }
  const float rstd = 1.0f / sqrtf(block_sum<4>(d2, red) / (float)C + p.eps);
  // LayerNorm backward: dx = rstd * (dy - mean(dy) - xhat * mean(dy * xhat)), dy = d out * weight
  const float sc = p.inv[tok];
  float dy[NV], s1 = 0.0f, s2 = 0.0f;
#pragma unroll
  for (int k = 0; k < NV; ++k) {
    const int c = tid + 256 * k;
    acc[k] *= rstd;                                   // xhat
    dy[k] = p.dxln[tok * C + c] * sc * p.ln_w[c];
    s1 += dy[k];
    s2 = fmaf(dy[k], acc[k], s2);
  }
  const float mdy = block_sum<4>(s1, red) / (float)C;
  const float mdyx = block_sum<4>(s2, red) / (float)C;
#pragma unroll
  for (int k = 0; k < NV; ++k) p.ddw[tok * C + tid + 256 * k] = rstd * (dy[k] - mdy - acc[k] * mdyx);
}

// forward: out(y, x) = sum_k in(y + ky - 3, x + kx - 3) w(ky, kx), so d in(y, x) = sum_k d out(y + 3 - ky, x + 3 - kx) w(ky, kx)
__global__ void __launch_bounds__(256) dw_dgrad_res_kernel(const float* __restrict__ ddw, const float* __restrict__ w,
                                                           float* g, int S, int C) {
  const int hw = S * S;
  const int64_t tok = blockIdx.x;
  const int img = (int)(tok / hw), q = (int)(tok - (int64_t)img * hw), y = q / S, x = q - y * S;
  const float* D = ddw + (int64_t)img * hw * C;
  for (int c = threadIdx.x; c < C; c += 256) {
    float acc = g[tok * C + c];
    for (int ky = 0; ky < 7; ++ky) {
      const int ny = y + 3 - ky;
      if (ny < 0 || ny >= S) continue;
      for (int kx = 0; kx < 7; ++kx) {
        const int nx = x + 3 - kx;
        if (nx < 0 || nx >= S) continue;
        acc = fmaf(D[(int64_t)(ny * S + nx) * C + c], w[(ky * 7 + kx) * C + c], acc);
      }
    }
    g[tok * C + c] = acc;
  }
}

// The same for the map sides stage 3 has (7: 224-pixel passes, 3: the 112-pixel pass): one thread per (image, channel) holds
// the channel's S x S gradient map and its 49 taps in registers; every loop is unrolled, so the zero-padding bounds are
// compile-time constants and the loads of a wave are 64 neighbouring channels.  Same summation order as the kernel above.
template <int S>
__global__ void __launch_bounds__(256) dw_dgrad_res_img_kernel(const float* __restrict__ ddw, const float* __restrict__ w,
                                                               float* g, int C) {
  const int c = blockIdx.y * 256 + threadIdx.x;               // C is a multiple of 256
  const int64_t base = (int64_t)blockIdx.x * (S * S) * C + c;
  float d[S * S], t[49];
#pragma unroll
  for (int q = 0; q < S * S; ++q) d[q] = ddw[base + (int64_t)q * C];
#pragma unroll
  for (int k = 0; k < 49; ++k) t[k] = w[k * C + c];
#pragma unroll
  for (int y = 0; y < S; ++y) {
#pragma unroll
    for (int x = 0; x < S; ++x) {
      float acc = g[base + (int64_t)(y * S + x) * C];
#pragma unroll
      for (int ky = 0; ky < 7; ++ky) {
#pragma unroll
        for (int kx = 0; kx < 7; ++kx) {
          const int ny = y + 3 - ky, nx = x + 3 - kx;
          if (ny >= 0 && ny < S && nx >= 0 && nx < S) acc = fmaf(d[ny * S + nx], t[ky * 7 + kx], acc);
        }
      }
      g[base + (int64_t)(y * S + x) * C] = acc;
    }
  }
}

// one workgroup of two waves per stage-2 token
template <typename T, int C2>
__global__ void __launch_bounds__(128) down_ln_bwd_kernel(DownLnBwdArgs p) {
  constexpr int NV = C2 / 128;
  __shared__ float red[2];
  const int tid = threadIdx.x, S = p.side2, hw = S * S, h2 = S / 2;
  const int64_t tok = blockIdx.x;
  const int img = (int)(tok / hw), q = (int)(tok - (int64_t)img * hw), y = q / S, x = q - y * S;
  float* out = p.dA2 + tok * C2;
  if (y >= 2 * h2 || x >= 2 * h2) {       // the odd last row / column takes no part in the forward (workgroup-uniform)
#pragma unroll
    for (int k = 0; k < NV; ++k) out[tid + 128 * k] = 0.0f;
    return;
  }
  const T* X = (const T*)p.x + tok * C2;
  float xv[NV], s0 = 0.0f;
#pragma unroll
  for (int k = 0; k < NV; ++k) { xv[k] = to_f(X[tid + 128 * k]); s0 += xv[k]; }
  const float mean = block_sum<2>(s0, red) / (float)C2;
  float d2 = 0.0f;
#pragma unroll
  for (int k = 0; k < NV; ++k) { xv[k] -= mean; d2 = fmaf(xv[k], xv[k], d2); }
  const float rstd = 1.0f / sqrtf(block_sum<2>(d2, red) / (float)C2 + p.eps);
  const int64_t row3 = (int64_t)img * h2 * h2 + (y >> 1) * h2 + (x >> 1);
  const float* dP = p.dP + row3 * (4 * C2) + ((y & 1) * 2 + (x & 1)) * C2;
  const float sc = p.inv[row3];
  float dy[NV], s1 = 0.0f, s2 = 0.0f;
#pragma unroll
  for (int k = 0; k < NV; ++k) {
    const int c = tid + 128 * k;
    xv[k] *= rstd;
    dy[k] = dP[c] * sc * p.ln_w[c];
    s1 += dy[k];
    s2 = fmaf(dy[k], xv[k], s2);
  }
  const float mdy = block_sum<2>(s1, red) / (float)C2;
  const float mdyx = block_sum<2>(s2, red) / (float)C2;
#pragma unroll
  for (int k = 0; k < NV; ++k) out[tid + 128 * k] = rstd * (dy[k] - mdy - xv[k] * mdyx);
}

// one workgroup per (frame, pass): a thread sums a channel's gradient over the map (neighbouring threads read neighbouring
// channels), then each wave takes every fourth stage-2 token's dot product with alpha
template <typename T, int C2>
__global__ void __launch_bounds__(256) cam2_kernel(Cam2Args p) {
  __shared__ float alpha[C2];
  __shared__ float map[196];
  const int b = blockIdx.x, pass = blockIdx.y, tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  const int S = p.side[pass], hw = S * S;
  const T* A = (const T*)p.A[pass] + (int64_t)b * hw * C2;
  const float* dA = p.dA2[pass] + (int64_t)b * hw * C2;
  const float inv = 1.0f / (float)hw;
  for (int c = tid; c < C2; c += 256) {
    float s = 0.0f;
    for (int q = 0; q < hw; ++q) s += dA[(int64_t)q * C2 + c];
    s *= inv;
    alpha[c] = s;
    p.alpha[((int64_t)pass * p.B + b) * C2 + c] = s;
  }
  __syncthreads();
  float* out = p.cam + (int64_t)b * p.cam_ld + p.cam_off[pass];
  for (int q = wv; q < hw; q += 4) {
    float acc = 0.0f;
#pragma unroll
    for (int i = 0; i < C2 / 64; ++i) {
      const int c = lane + 64 * i;
      acc = fmaf(alpha[c], to_f(A[(int64_t)q * C2 + c]), acc);
    }
    acc = fmaxf(wave_sum(acc), 0.0f);
    if (lane == 0) { out[q] = acc; map[q] = acc; }
  }
  if (!p.cam224 || pass != p.up_pass) return;
  __syncthreads();
  // F.interpolate(size=(224, 224), mode='bilinear', align_corners=False): src = (dst + 0.5) * in / out - 0.5, clamped at 0
  const float sc = (float)S / 224.0f;
  float* up = p.cam224 + (int64_t)b * 224 * 224;
  for (int pix = tid; pix < 224 * 224; pix += 256) {
    const int oy = pix / 224, ox = pix - oy * 224;
    const float sy = fmaxf((oy + 0.5f) * sc - 0.5f, 0.0f), sx = fmaxf((ox + 0.5f) * sc - 0.5f, 0.0f);
    const int y0 = min((int)sy, S - 1), x0 = min((int)sx, S - 1);
    const int y1 = min(y0 + 1, S - 1), x1 = min(x0 + 1, S - 1);
    const float ly = sy - y0, lx = sx - x0;
    const float r0 = map[y0 * S + x0] * (1.0f - lx) + map[y0 * S + x1] * lx;
    const float r1 = map[y1 * S + x0] * (1.0f - lx) + map[y1 * S + x1] * lx;
    up[pix] = r0 * (1.0f - ly) + r1 * ly;
  }
}

// ---------------------------------------------------------------- launchers
template <typename T> int launch_pool_ln_bwd(const PoolLnBwdArgs& a, int C, hipStream_t s) {
  GCV_REQUIRE(a.B > 0 && a.npass >= 1 && a.npass <= 2 && (C == 768 || C == 1536), "pool_ln_bwd: empty, or C not 768 / 1536");
  for (int q = 0; q < a.npass; ++q) GCV_REQUIRE(a.A[q] && a.hw[q] >= 1 && a.tok0[q] >= 0, "pool_ln_bwd: pass geometry");
  GCV_REQUIRE(a.dA && a.dpool && a.lnw, "pool_ln_bwd: null operand");
  if (C == 768) hipLaunchKernelGGL((pool_ln_bwd_kernel<T, 768>), dim3(a.B, a.npass), dim3(256), 0, s, a);
  else hipLaunchKernelGGL((pool_ln_bwd_kernel<T, 1536>), dim3(a.B, a.npass), dim3(256), 0, s, a);
  GCV_CHECK_HIP(hipGetLastError());
  return 0;
}

template <typename T> int launch_scale_rows(const float* g, const float* gamma, T* out, float* inv, int M, int C, hipStream_t s) {
  GCV_REQUIRE(M > 0 && g && out && inv && (C == 768 || C == 1536), "scale_rows: empty, or C not 768 / 1536");
  if (C == 768) hipLaunchKernelGGL((scale_rows_kernel<T, 3>), dim3(M), dim3(256), 0, s, g, gamma, out, inv);
  else hipLaunchKernelGGL((scale_rows_kernel<T, 6>), dim3(M), dim3(256), 0, s, g, gamma, out, inv);
  GCV_CHECK_HIP(hipGetLastError());
  return 0;
}

template <typename T> int launch_gelu_bwd(const float* dh, const float* inv_in, T* pre, float* inv_out, int M, int C4, hipStream_t s) {
  GCV_REQUIRE(M > 0 && dh && inv_in && pre && inv_out && (C4 == 3072 || C4 == 6144), "gelu_bwd: empty, or 4C not 3072 / 6144");
  if (C4 == 3072) hipLaunchKernelGGL((gelu_bwd_kernel<T, 12>), dim3(M), dim3(256), 0, s, dh, inv_in, pre, inv_out);
  else hipLaunchKernelGGL((gelu_bwd_kernel<T, 24>), dim3(M), dim3(256), 0, s, dh, inv_in, pre, inv_out);
  GCV_CHECK_HIP(hipGetLastError());
  return 0;
}

template <typename T> int launch_dw_ln_bwd(const DwLnBwdArgs& a, int C, hipStream_t s) {
  GCV_REQUIRE(a.nimg > 0 && a.side >= 1 && a.side <= 7 && (C == 768 || C == 1536), "dw_ln_bwd: map of at most 7 x 7, C 768 / 1536");
  GCV_REQUIRE(a.x && a.dw_w && a.dw_b && a.ln_w && a.dxln && a.inv && a.ddw, "dw_ln_bwd: null operand");
  const dim3 grid(a.nimg * a.side * a.side);
  if (C == 768) hipLaunchKernelGGL((dw_ln_bwd_kernel<T, 768>), grid, dim3(256), 0, s, a);
  else hipLaunchKernelGGL((dw_ln_bwd_kernel<T, 1536>), grid, dim3(256), 0, s, a);
  GCV_CHECK_HIP(hipGetLastError());
  return 0;
}

int launch_dw_dgrad_res(const float* ddw, const float* dw_w, float* g, int nimg, int side, int C, hipStream_t s) {
  GCV_REQUIRE(nimg > 0 && side >= 1 && side <= 7 && C > 0 && ddw && dw_w && g, "dw_dgrad_res: map of at most 7 x 7");
  if (side == 7 && C % 256 == 0)
    hipLaunchKernelGGL(dw_dgrad_res_img_kernel<7>, dim3(nimg, C / 256), dim3(256), 0, s, ddw, dw_w, g, C);
  else if (side == 3 && C % 256 == 0)
    hipLaunchKernelGGL(dw_dgrad_res_img_kernel<3>, dim3(nimg, C / 256), dim3(256), 0, s, ddw, dw_w, g, C);
  else
    hipLaunchKernelGGL(dw_dgrad_res_kernel, dim3(nimg * side * side), dim3(256), 0, s, ddw, dw_w, g, side, C);
  GCV_CHECK_HIP(hipGetLastError());
  return 0;
}

template <typename T> int launch_down_ln_bwd(const DownLnBwdArgs& a, int C2, hipStream_t s) {
  GCV_REQUIRE(a.nimg > 0 && a.side2 >= 2 && a.side2 <= 14 && (C2 == 384 || C2 == 768), "down_ln_bwd: map of 2..14, C2 384 / 768");
  GCV_REQUIRE(a.x && a.ln_w && a.dP && a.inv && a.dA2, "down_ln_bwd: null operand");
  const dim3 grid(a.nimg * a.side2 * a.side2);
  if (C2 == 384) hipLaunchKernelGGL((down_ln_bwd_kernel<T, 384>), grid, dim3(128), 0, s, a);
  else hipLaunchKernelGGL((down_ln_bwd_kernel<T, 768>), grid, dim3(128), 0, s, a);
  GCV_CHECK_HIP(hipGetLastError());
  return 0;
}

template <typename T> int launch_cam2(const Cam2Args& a, int C2, hipStream_t s) {
  GCV_REQUIRE(a.B > 0 && a.npass >= 1 && a.npass <= 2 && (C2 == 384 || C2 == 768), "cam2: empty, or C2 not 384 / 768");
  for (int q = 0; q < a.npass; ++q)
    GCV_REQUIRE(a.A[q] && a.dA2[q] && a.side[q] >= 1 && a.side[q] <= 14, "cam2: stage-2 map of at most 14 x 14");
  GCV_REQUIRE(a.cam && a.alpha, "cam2: null output");
  if (C2 == 384) hipLaunchKernelGGL((cam2_kernel<T, 384>), dim3(a.B, a.npass), dim3(256), 0, s, a);
  else hipLaunchKernelGGL((cam2_kernel<T, 768>), dim3(a.B, a.npass), dim3(256), 0, s, a);
  GCV_CHECK_HIP(hipGetLastError());
  return 0;
}

#define GCV_INSTANTIATE_CAM_BWD(T)                                                                   \
  template int launch_pool_ln_bwd<T>(const PoolLnBwdArgs&, int, hipStream_t);                        \
  template int launch_scale_rows<T>(const float*, const float*, T*, float*, int, int, hipStream_t);  \
  template int launch_gelu_bwd<T>(const float*, const float*, T*, float*, int, int, hipStream_t);    \
  template int launch_dw_ln_bwd<T>(const DwLnBwdArgs&, int, hipStream_t);                            \
  template int launch_down_ln_bwd<T>(const DownLnBwdArgs&, int, hipStream_t);                        \
  template int launch_cam2<T>(const Cam2Args&, int, hipStream_t);
GCV_INSTANTIATE_CAM_BWD(float)
GCV_INSTANTIATE_CAM_BWD(half_t)
GCV_INSTANTIATE_CAM_BWD(bf16_t)
#undef GCV_INSTANTIATE_CAM_BWD

}  // namespace gcv
