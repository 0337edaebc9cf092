// Grad-CAM kernels (cam.h), instantiated for the three storage dtypes.
#include "cam.h"

namespace gcv {

// derivative of the head's activation at the pre-activation x (nn.GELU exact-erf / nn.ReLU; ReLU'(0) = 0 as in autograd)
template <int ACT> __device__ __forceinline__ float act_grad(float x) {
  if constexpr (ACT == ACT_GELU)
    return 0.5f * (1.0f + erff(x * 0.70710678118654752440f)) + x * 0.39894228040143267794f * __expf(-0.5f * x * x);
  else
    return x > 0.0f ? 1.0f : 0.0f;
}

// out[r][j] = sum_k a[r][k] * W[k][j] for RB rows r and 64 columns j per workgroup, W (K, N) row-major in T: the lanes of
// a wave read 64 consecutive columns of one weight row, each weight element serves RB rows, the rows' coefficients are
// wave-uniform LDS reads, and the four waves take a quarter of K each (eight loads in flight per lane) and meet in LDS.
// Every thread reaches the barrier; the sum lands in wave 0.  K % 4 == 0.
constexpr int kRB = 8;
template <typename T, int KMAX>
__device__ __forceinline__ void tn_rows(const float (&a)[kRB][KMAX], float (&red)[4][kRB][64], const T* __restrict__ W,
                                        int K, int N, int j, float (&acc)[kRB]) {
  const int wv = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const int kc = ((K + 15) / 16) * 4, k0 = wv * kc, k1 = min(K, k0 + kc);
#pragma unroll
  for (int f = 0; f < kRB; ++f) acc[f] = 0.0f;
  if (j < N) {
#pragma unroll 2
    for (int k = k0; k < k1; k += 4) {
      float w[4];
#pragma unroll
      for (int u = 0; u < 4; ++u) w[u] = to_f(W[(int64_t)(k + u) * N + j]);
#pragma unroll
      for (int f = 0; f < kRB; ++f) {
        const float4 c = *reinterpret_cast<const float4*>(&a[f][k]);
        acc[f] = fmaf(c.x, w[0], acc[f]);
        acc[f] = fmaf(c.y, w[1], acc[f]);
        acc[f] = fmaf(c.z, w[2], acc[f]);
        acc[f] = fmaf(c.w, w[3], acc[f]);
      }
    }
  }
#pragma unroll
  for (int f = 0; f < kRB; ++f) red[wv][f][lane] = acc[f];
  __syncthreads();
#pragma unroll
  for (int f = 0; f < kRB; ++f) acc[f] = red[0][f][lane] + red[1][f][lane] + red[2][f][lane] + red[3][f][lane];
}

template <typename T, int ACT>
__global__ void __launch_bounds__(256) head_bwd_kernel(HeadBwdArgs p) {
  constexpr int K = 500, N = 2000;
  __shared__ __attribute__((aligned(16))) float a[kRB][K];
  __shared__ float red[4][kRB][64];
  const int tid = threadIdx.x, r0 = blockIdx.x * kRB;
  // d logit / d hidden pre-activation: fc2 row of the target class times act'; the pre-activation is the forward's own
  // split-K sum (same partials, same order)
  for (int i = tid; i < kRB * K; i += 256) {
    const int f = i / K, k = i - f * K, b = r0 + f;
    float v = 0.0f;
    if (b < p.B) {
      float h = p.b1[k];
      for (int s = 0; s < p.S; ++s) h += p.partial[((int64_t)s * p.B + b) * K + k];
      const int t = p.target ? (p.target[b] != 0) : (p.logits[2 * b + 1] > p.logits[2 * b]);
      v = p.fc2_w[t * K + k] * act_grad<ACT>(h);
    }
    a[f][k] = v;
  }
  __syncthreads();
  const int j = blockIdx.y * 64 + (tid & 63);
  float acc[kRB];
  tn_rows<T, K>(a, red, (const T*)p.fc_w, K, N, j, acc);
  if (tid >= 64 || j >= N) return;
  const T* pre = (const T*)p.bb_pre;
#pragma unroll
  for (int f = 0; f < kRB; ++f) {
    const int b = r0 + f;
    if (b < p.B) p.dfeat[(int64_t)b * N + j] = acc[f] * act_grad<ACT>(to_f(pre[(int64_t)b * N + j]));
  }
}

template <typename T, int N = 768>
__global__ void __launch_bounds__(256) bb_bwd_kernel(const float* __restrict__ dfeat, const T* __restrict__ W,
                                                     float* __restrict__ dpool, int rows) {
  constexpr int K = 1000;
  __shared__ __attribute__((aligned(16))) float a[kRB][K];
  __shared__ float red[4][kRB][64];
  const int tid = threadIdx.x, r0 = blockIdx.x * kRB;
  for (int i = tid; i < kRB * K; i += 256) {
    const int f = i / K, k = i - f * K;
    a[f][k] = r0 + f < rows ? dfeat[(int64_t)(r0 + f) * K + k] : 0.0f;
  }
  __syncthreads();
  const int j = blockIdx.y * 64 + (tid & 63);
  float acc[kRB];
  tn_rows<T, K>(a, red, W, K, N, j, acc);
  if (tid >= 64 || j >= N) return;
#pragma unroll
  for (int f = 0; f < kRB; ++f)
    if (r0 + f < rows) dpool[(int64_t)(r0 + f) * N + j] = acc[f];
}

// sum over the 256 threads of a workgroup (4 waves); `red` holds 4 floats, reused after the call's barrier pair
__device__ __forceinline__ float block_sum256(float v, float* red) {
  v = wave_sum(v);
  __syncthreads();
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
  __syncthreads();
  return red[0] + red[1] + red[2] + red[3];
}

// one workgroup per (frame, pass): four waves share the LayerNorm backward, then each wave takes every fourth stage-3
// token and reduces its C-channel dot product with g across the wave (DPP rows + two cross-row steps); C = 768 (ConvNeXt-T)
// or 1536 (ConvNeXt-L), NV = C / 256 channels per thread
template <typename T, int C = 768>
__global__ void __launch_bounds__(256) cam_kernel(CamArgs p) {
  constexpr int NV = C / 256;
  __shared__ float g[C];
  __shared__ float red[4];
  __shared__ float map[49];
  const int b = blockIdx.x, pass = blockIdx.y, tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  const int hw = p.hw[pass];
  const T* A = (const T*)p.A[pass] + (int64_t)b * hw * C;
  // the pooled row and its LayerNorm statistics, as pool_ln_kernel computes them
  float m[NV];
#pragma unroll
  for (int k = 0; k < NV; ++k) m[k] = 0.0f;
  for (int q = 0; q < hw; ++q) {
#pragma unroll
    for (int k = 0; k < NV; ++k) m[k] += to_f(A[(int64_t)q * C + tid + 256 * k]);
  }
  const float inv = 1.0f / (float)hw;
#pragma unroll
  for (int k = 0; k < NV; ++k) m[k] *= inv;
  float msum = m[0];
#pragma unroll
  for (int k = 1; k < NV; ++k) msum += m[k];
  const float mean = block_sum256(msum, red) / (float)C;
  float d2 = 0.0f;
#pragma unroll
  for (int k = 0; k < NV; ++k) { const float d = m[k] - mean; d2 = fmaf(d, d, d2); }
  const float rstd = 1.0f / sqrtf(block_sum256(d2, red) / (float)C + p.eps);
  // LayerNorm backward: dx = rstd * (dy - mean(dy) - xhat * mean(dy * xhat)), dy = d out * weight; the pooled row's
  // gradient spreads evenly over the hw tokens
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
  const float mdy = block_sum256(s1, red) / (float)C;
  const float mdyx = block_sum256(s2, red) / (float)C;
#pragma unroll
  for (int k = 0; k < NV; ++k) g[tid + 256 * k] = rstd * (dy[k] - mdy - xh[k] * mdyx) * inv;
  __syncthreads();
  float* out = p.cam + (int64_t)b * p.cam_ld + p.cam_off[pass];
  for (int q = wv; q < hw; q += 4) {
    float acc = 0.0f;
#pragma unroll
    for (int i = 0; i < C / 64; ++i) {
      const int c = lane + 64 * i;
      acc = fmaf(g[c], to_f(A[(int64_t)q * C + c]), acc);
    }
    acc = fmaxf(wave_sum(acc), 0.0f);
    if (lane == 0) { out[q] = acc; map[q] = acc; }
  }
  if (!p.cam224 || pass != p.up_pass) return;
  __syncthreads();
  // F.interpolate(size=(224, 224), mode='bilinear', align_corners=False): src = (dst + 0.5) * in / out - 0.5, clamped at 0
  const int S = p.side[pass];
  const float sc = (float)S / 224.0f;
  float* up = p.cam224 + (int64_t)b * 224 * 224;
  for (int pix = tid; pix < 224 * 224; pix += 256) {
    const int oy = pix / 224, ox = pix - oy * 224;
    const float sy = fmaxf((oy + 0.5f) * sc - 0.5f, 0.0f), sx = fmaxf((ox + 0.5f) * sc - 0.5f, 0.0f);
    const int y0 = (int)sy, x0 = (int)sx;
    const int y1 = min(y0 + 1, S - 1), x1 = min(x0 + 1, S - 1);
    const float ly = sy - y0, lx = sx - x0;
    const float r0 = map[y0 * S + x0] * (1.0f - lx) + map[y0 * S + x1] * lx;
    const float r1 = map[y1 * S + x0] * (1.0f - lx) + map[y1 * S + x1] * lx;
    up[pix] = r0 * (1.0f - ly) + r1 * ly;
  }
}

template <typename T> int launch_head_bwd(const HeadBwdArgs& a, hipStream_t s) {
  GCV_REQUIRE(a.B > 0 && a.S >= 1, "head_bwd: empty");
  GCV_REQUIRE(a.partial && a.b1 && a.fc2_w && (a.target || a.logits) && a.fc_w && a.bb_pre && a.dfeat, "head_bwd: null operand");
  const dim3 grid(cdiv(a.B, kRB), cdiv(2000, 64));
  if (a.act == ACT_GELU) hipLaunchKernelGGL((head_bwd_kernel<T, ACT_GELU>), grid, dim3(256), 0, s, a);
  else if (a.act == ACT_RELU) hipLaunchKernelGGL((head_bwd_kernel<T, ACT_RELU>), grid, dim3(256), 0, s, a);
  else { set_error("head_bwd: activation must be GELU or ReLU"); return -2; }
  GCV_CHECK_HIP(hipGetLastError());
  return 0;
}

template <typename T> int launch_bb_bwd(const float* dfeat, const void* W, float* dpool, int rows, int C, hipStream_t s) {
  GCV_REQUIRE(rows > 0 && (C == 768 || C == 1536), "bb_bwd: empty, or C not 768 / 1536");
  GCV_REQUIRE(dfeat && W && dpool, "bb_bwd: null operand");
  if (C == 768)
    hipLaunchKernelGGL((bb_bwd_kernel<T, 768>), dim3(cdiv(rows, kRB), 768 / 64), dim3(256), 0, s, dfeat, (const T*)W, dpool, rows);
  else
    hipLaunchKernelGGL((bb_bwd_kernel<T, 1536>), dim3(cdiv(rows, kRB), 1536 / 64), dim3(256), 0, s, dfeat, (const T*)W, dpool, rows);
  GCV_CHECK_HIP(hipGetLastError());
  return 0;
}

template <typename T> int launch_cam(const CamArgs& a, int C, hipStream_t s) {
  GCV_REQUIRE(a.B > 0 && a.npass >= 1 && a.npass <= 2 && (C == 768 || C == 1536), "cam: empty, or C not 768 / 1536");
  for (int q = 0; q < a.npass; ++q)
    GCV_REQUIRE(a.A[q] && a.side[q] >= 1 && a.side[q] * a.side[q] == a.hw[q] && a.hw[q] <= 49, "cam: stage-3 map of at most 7 x 7");
  GCV_REQUIRE(a.lnw && a.dpool && a.cam, "cam: null operand");
  if (C == 768) hipLaunchKernelGGL((cam_kernel<T, 768>), dim3(a.B, a.npass), dim3(256), 0, s, a);
  else hipLaunchKernelGGL((cam_kernel<T, 1536>), dim3(a.B, a.npass), dim3(256), 0, s, a);
  GCV_CHECK_HIP(hipGetLastError());
  return 0;
}

#define GCV_INSTANTIATE_CAM(T)                                                          \
  template int launch_head_bwd<T>(const HeadBwdArgs&, hipStream_t);                     \
  template int launch_bb_bwd<T>(const float*, const void*, float*, int, int, hipStream_t); \
  template int launch_cam<T>(const CamArgs&, int, hipStream_t);
GCV_INSTANTIATE_CAM(float)
GCV_INSTANTIATE_CAM(half_t)
GCV_INSTANTIATE_CAM(bf16_t)
#undef GCV_INSTANTIATE_CAM

}  // namespace gcv
