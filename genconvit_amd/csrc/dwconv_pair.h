// K4 at the ConvNeXt-L widths: depthwise 7x7 + LayerNorm where C * W / 7 = 1536, two channels per lane.
//
// Every 224-pixel stage of ConvNeXt-L has NS * C = 1536 with NS = W / 7: (192, 56), (384, 28), (768, 14), (1536, 7).  The
// rolling-strip kernel (dwconv_roll.h) runs one tap thread per (7-pixel strip, channel), at most 768 of them, and the generic
// tile kernel launches one thread per channel; neither takes 1536 lanes of work.  Here a workgroup of 768 threads covers a
// whole image row: thread = (strip sl, channel pair cp), NS strips x C / 2 pairs.  A thread keeps the 98 fp32 taps of its
// two channels in registers for the whole band of output rows it walks; per output row it reads the 7 input rows' 13
// halo columns of its strip as packed pairs (4 bytes in 16-bit storage, 8 in fp32) straight from memory — neighbouring
// lanes read neighbouring pairs, and the 7 x 13 re-reads of an input value come from L1 / L2 — and accumulates its 7
// pixels x 2 channels in fp32.  LayerNorm over the C channels of a pixel: the strip's C / 2 lanes reduce in 32-lane groups
// into LDS, mean first, then the centred second moment (two passes).  Rows above / below the image are skipped by
// wave-uniform branches; at NS = 1 the columns outside the 7-pixel image are skipped at compile time.
//
// dwconv7_ln_tiny2_kernel: the same two-channels-per-lane layout for maps of at most 4 x 4 (the 3 x 3 stage-3 map of the
// 112-pixel pass at C = 1536), after dwconv7_ln_tiny_kernel: one workgroup per image, inputs, outputs and taps in registers.
#pragma once
#include "common.h"

namespace gcv {

// two storage values <-> a packed pair: 4 bytes in 16-bit storage, 8 in fp32
template <typename T> struct DwPair;
template <> struct DwPair<float> {
  typedef float2 raw;
  __device__ static __forceinline__ float lo(raw v) { return v.x; }
  __device__ static __forceinline__ float hi(raw v) { return v.y; }
  __device__ static __forceinline__ raw pack(float a, float b) { return make_float2(a, b); }
};
template <typename T> struct DwPair16 {
  typedef uint32_t raw;
  __device__ static __forceinline__ float lo(raw v) { return to_f(__builtin_bit_cast(T, (unsigned short)(v & 0xffffu))); }
  __device__ static __forceinline__ float hi(raw v) { return to_f(__builtin_bit_cast(T, (unsigned short)(v >> 16))); }
  __device__ static __forceinline__ raw pack(float a, float b) {
    return (uint32_t)__builtin_bit_cast(unsigned short, from_f<T>(a)) |
           ((uint32_t)__builtin_bit_cast(unsigned short, from_f<T>(b)) << 16);
  }
};
template <> struct DwPair<half_t> : DwPair16<half_t> {};
template <> struct DwPair<bf16_t> : DwPair16<bf16_t> {};

constexpr int kDwPairThreads = 768;

// grid: nimg * nbands workgroups of 768 threads; workgroup = (image, band of `band_rows` output rows)
template <typename T, int C, int NS>
__global__ void __launch_bounds__(kDwPairThreads)
dwconv7_ln_pair_kernel(const T* __restrict__ x, const float* __restrict__ wdw /*[49][C]*/, const float* __restrict__ bdw,
                       const float* __restrict__ lnw, const float* __restrict__ lnb, T* __restrict__ y, int H, int band_rows,
                       int nbands, float eps) {
  static_assert(NS * C == 2 * kDwPairThreads && C % 64 == 0, "NS strips x C / 2 channel pairs = 768 lanes");
  typedef DwPair<T> PR;
  typedef typename PR::raw raw;
  constexpr int W = 7 * NS, CP = C / 2, NG = CP / 32;   // NG 32-lane groups per strip
  constexpr int S0 = (NS == 1) ? 3 : 0, S1 = (NS == 1) ? 10 : 13;   // halo columns that can hold data
  __shared__ float red[2][NS * NG][7];
  __shared__ float tot[2][NS][7];                        // per (strip, pixel): mean, then rstd
  const int tid = threadIdx.x;
  const int sl = tid / CP, cp = tid - sl * CP, c0 = 2 * cp;
  const int grp = tid >> 5;                              // = sl * NG + cp / 32
  const int band = blockIdx.x % nbands, img = blockIdx.x / nbands;
  const int ob = band * band_rows, oe = min(H, ob + band_rows);
  const int64_t img_elems = (int64_t)H * W * C;
  const raw* xi = reinterpret_cast<const raw*>(x + (int64_t)img * img_elems + c0);
  raw* yi = reinterpret_cast<raw*>(y + (int64_t)img * img_elems + c0);
  constexpr int ROWP = W * C / 2, PIXP = C / 2;          // pairs per row / per pixel

  float w0[49], w1[49];
#pragma unroll
  for (int k = 0; k < 49; ++k) {
    const float2 t = *reinterpret_cast<const float2*>(wdw + k * C + c0);
    w0[k] = t.x; w1[k] = t.y;
  }
  const float2 bv = *reinterpret_cast<const float2*>(bdw + c0);
  const float2 lw = *reinterpret_cast<const float2*>(lnw + c0);
  const float2 lb = *reinterpret_cast<const float2*>(lnb + c0);
  // halo column s of this strip is image column 7 sl - 3 + s
  bool col_ok[13];
#pragma unroll
  for (int s = 0; s < 13; ++s) col_ok[s] = s >= S0 && s < S1 && 7 * sl - 3 + s >= 0 && 7 * sl - 3 + s < W;

  for (int oy = ob; oy < oe; ++oy) {
    float a0[7], a1[7];
#pragma unroll
    for (int p = 0; p < 7; ++p) { a0[p] = bv.x; a1[p] = bv.y; }
#pragma unroll
    for (int ky = 0; ky < 7; ++ky) {
      const int r = oy + ky - 3;
      if (r < 0 || r >= H) continue;                     // wave-uniform
      float i0[13], i1[13];
      const raw* xr = xi + (int64_t)r * ROWP + (int64_t)(7 * sl - 3) * PIXP;
#pragma unroll
      for (int s = S0; s < S1; ++s) {
        raw v{};
        if (NS == 1 || col_ok[s]) v = xr[s * PIXP];
        i0[s] = PR::lo(v); i1[s] = PR::hi(v);
      }
#pragma unroll
      for (int ox = 0; ox < 7; ++ox)
#pragma unroll
        for (int kx = 0; kx < 7; ++kx)
          if (ox + kx >= S0 && ox + kx < S1) {
            a0[ox] = fmaf(i0[ox + kx], w0[ky * 7 + kx], a0[ox]);
            a1[ox] = fmaf(i1[ox + kx], w1[ky * 7 + kx], a1[ox]);
          }
      // one tap row's 13 loads in flight at a time: hoisting all seven rows' loads costs more registers than the 98 taps
      // leave (768 threads: 168 VGPRs per lane)
      __builtin_amdgcn_sched_barrier(0);
    }
    // LayerNorm over the C channels of each of the strip's 7 pixels: mean, then the centred second moment.  32-lane sums
    // into LDS, then one thread per (strip, pixel) adds its strip's NG of them (every lane summing them itself kept
    // 7 * NG values live at C = 1536)
    float mean[7];
#pragma unroll
    for (int p = 0; p < 7; ++p) {
      const float s = group32_sum(a0[p] + a1[p]);
      if ((tid & 31) == 0) red[0][grp][p] = s;
    }
    __syncthreads();
    if (tid < NS * 7) {
      const int ts = tid / 7, tp = tid - ts * 7;
      float t = 0.0f;
      for (int g = 0; g < NG; ++g) t += red[0][ts * NG + g][tp];
      tot[0][ts][tp] = t * (1.0f / C);
    }
    __syncthreads();
#pragma unroll
    for (int p = 0; p < 7; ++p) {
      mean[p] = tot[0][sl][p];
      const float d0 = a0[p] - mean[p], d1 = a1[p] - mean[p];
      const float q = group32_sum(fmaf(d0, d0, d1 * d1));
      if ((tid & 31) == 0) red[1][grp][p] = q;
    }
    __syncthreads();
    if (tid < NS * 7) {
      const int ts = tid / 7, tp = tid - ts * 7;
      float t = 0.0f;
      for (int g = 0; g < NG; ++g) t += red[1][ts * NG + g][tp];
      tot[1][ts][tp] = 1.0f / sqrtf(t * (1.0f / C) + eps);
    }
    __syncthreads();
    raw* yr = yi + (int64_t)oy * ROWP + (int64_t)(7 * sl) * PIXP;
#pragma unroll
    for (int p = 0; p < 7; ++p) {
      const float rstd = tot[1][sl][p];
      yr[p * PIXP] = PR::pack(fmaf((a0[p] - mean[p]) * rstd, lw.x, lb.x), fmaf((a1[p] - mean[p]) * rstd, lw.y, lb.y));
    }
  }
}

// S x S maps, S <= 4: one workgroup per image, C / 2 threads of two channels each
template <typename T, int C, int S>
__global__ void __launch_bounds__(C / 2) dwconv7_ln_tiny2_kernel(const T* __restrict__ x, const float* __restrict__ wdw /*[49][C]*/,
                                                                 const float* __restrict__ bdw, const float* __restrict__ lnw,
                                                                 const float* __restrict__ lnb, T* __restrict__ y, float eps) {
  static_assert(S >= 1 && S <= 4 && C % 128 == 0 && C / 2 <= 1024, "tiny maps, whole waves of channel pairs");
  typedef DwPair<T> PR;
  typedef typename PR::raw raw;
  constexpr int NPX = S * S, NW = C / 128, CP = C / 2;
  __shared__ float part[2][NW][NPX];
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63, c0 = 2 * tid;
  const raw* xb = reinterpret_cast<const raw*>(x + (int64_t)blockIdx.x * NPX * C + c0);
  float i0[NPX], i1[NPX], a0[NPX], a1[NPX];
#pragma unroll
  for (int p = 0; p < NPX; ++p) { const raw v = xb[p * CP]; i0[p] = PR::lo(v); i1[p] = PR::hi(v); }
  const float2 bv = *reinterpret_cast<const float2*>(bdw + c0);
#pragma unroll
  for (int p = 0; p < NPX; ++p) { a0[p] = bv.x; a1[p] = bv.y; }
#pragma unroll
  for (int dy = -(S - 1); dy <= S - 1; ++dy)
#pragma unroll
    for (int dx = -(S - 1); dx <= S - 1; ++dx) {
      const float2 w = *reinterpret_cast<const float2*>(wdw + ((dy + 3) * 7 + dx + 3) * C + c0);
#pragma unroll
      for (int oy = 0; oy < S; ++oy)
#pragma unroll
        for (int ox = 0; ox < S; ++ox)
          if (oy + dy >= 0 && oy + dy < S && ox + dx >= 0 && ox + dx < S) {
            a0[oy * S + ox] = fmaf(i0[(oy + dy) * S + ox + dx], w.x, a0[oy * S + ox]);
            a1[oy * S + ox] = fmaf(i1[(oy + dy) * S + ox + dx], w.y, a1[oy * S + ox]);
          }
    }
  float mean[NPX];
#pragma unroll
  for (int p = 0; p < NPX; ++p) {
    const float sp = wave_sum(a0[p] + a1[p]);
    if (lane == 0) part[0][wave][p] = sp;
  }
  __syncthreads();
#pragma unroll
  for (int p = 0; p < NPX; ++p) {
    float t = 0.0f;
#pragma unroll
    for (int w = 0; w < NW; ++w) t += part[0][w][p];
    mean[p] = t * (1.0f / C);
    const float d0 = a0[p] - mean[p], d1 = a1[p] - mean[p];
    const float qp = wave_sum(fmaf(d0, d0, d1 * d1));
    if (lane == 0) part[1][wave][p] = qp;
  }
  __syncthreads();
  const float2 lw = *reinterpret_cast<const float2*>(lnw + c0);
  const float2 lb = *reinterpret_cast<const float2*>(lnb + c0);
  raw* yb = reinterpret_cast<raw*>(y + (int64_t)blockIdx.x * NPX * C + c0);
#pragma unroll
  for (int p = 0; p < NPX; ++p) {
    float t = 0.0f;
#pragma unroll
    for (int w = 0; w < NW; ++w) t += part[1][w][p];
    const float rs = 1.0f / sqrtf(t * (1.0f / C) + eps);
    yb[p * CP] = PR::pack(fmaf((a0[p] - mean[p]) * rs, lw.x, lb.x), fmaf((a1[p] - mean[p]) * rs, lw.y, lb.y));
  }
}

}  // namespace gcv
