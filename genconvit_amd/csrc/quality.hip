// Is a face crop usable: sharpness, gradient and exposure sums of n face boxes on a G x G grid of mean-luma cells
// (gcv_face_quality, include/genconvit_hip.h, which fixes the arithmetic; tests/qualityutil.py restates it bit for bit).
// A whole-video scan scores every face of every frame; a crop smeared by motion or defocus, blown out by a flash or lost in
// the dark is no evidence, and pred_func.quality_keep takes it out of the votes by the numbers this returns.
//
// One workgroup per box, three phases:
//   1. the cells as bytes in LDS.  One thread = one cell; consecutive lanes take consecutive cells of a cell row, so a
//      wave's reads of one pixel row are one contiguous run of RGB bytes (follow.hip, phase 1; the cell is its tm_cell).
//   2. cell i = tid + 256 k goes to lane tid: a wave reads 64 consecutive bytes of a cell row — 16 dwords on 16 banks, the
//      four lanes of a dword at the same bank row — and the rows above and below alike, so no read conflicts.  A lane
//      adds its cells' terms of the seven sums in 32 bits: 16 cells at the most, 16 * 1020^2 < 2^24 for the largest term.
//   3. each sum across the wave by shuffles, still in 32 bits (64 * 16 * 1020^2 < 2^31), across the four waves through LDS
//      in 64; one lane stores the row.
// No atomics, no scratch, nothing allocated or synchronised.
#include <cstdint>

#include "common.h"
#include "luma_cells.h"                                   // TmBox, tm_box_ok, tm_cell

namespace gcv {

constexpr int FQ_THREADS = 256;
constexpr int FQ_SUMS = 7;                                // S1, S2, L2, GX, GY, dark, bright

struct alignas(8) FqOut { long long v[8]; };

template <int G>
__global__ void __launch_bounds__(FQ_THREADS) face_quality_kernel(const unsigned char* __restrict__ frames, int nframes,
                                                                  int H, int W, const int* __restrict__ boxes,
                                                                  long long* __restrict__ out) {
  constexpr int LG = G == 16 ? 4 : (G == 32 ? 5 : 6);
  __shared__ __attribute__((aligned(16))) unsigned char s_c[G * G];
  __shared__ int s_ey[G + 1], s_ex[G + 1];
  __shared__ unsigned s_part[FQ_THREADS / 64][FQ_SUMS];

  const int tid = threadIdx.x;
  const int* j = boxes + 5 * (size_t)blockIdx.x;
  const TmBox p = {j[0], j[1], j[2], j[3], j[4]};
  FqOut* dst = reinterpret_cast<FqOut*>(out + 8 * (size_t)blockIdx.x);
  // a bad row (block-uniform): read nothing, write zeros
  if (!tm_box_ok(p, nframes, H, W, G)) {
    if (tid == 0) *dst = FqOut{{0, 0, 0, 0, 0, 0, 0, 0}};
    return;
  }
  const int h = p.bottom - p.top, w = p.right - p.left;
  for (int i = tid; i <= G; i += FQ_THREADS) {
    s_ey[i] = (int)(((int64_t)i * h) >> LG);
    s_ex[i] = (int)(((int64_t)i * w) >> LG);
  }
  __syncthreads();

  // phase 1: the cells.  The box lies inside the frame and the cells tile it, so no byte outside the frames is read
  {
    const int64_t rs = (int64_t)W * 3;
    const unsigned char* frame = frames + (int64_t)p.f * H * rs;
    for (int i = tid; i < G * G; i += FQ_THREADS) {
      const int u = i >> LG, v = i & (G - 1);
      s_c[i] = (unsigned char)tm_cell(frame, rs, p.top + s_ey[u], p.top + s_ey[u + 1], p.left + s_ex[v],
                                      p.left + s_ex[v + 1]);
    }
  }
  __syncthreads();

  // phase 2: a lane's terms
  unsigned acc[FQ_SUMS] = {0, 0, 0, 0, 0, 0, 0};
#pragma unroll
  for (int i0 = 0; i0 < G * G; i0 += FQ_THREADS) {
    const int i = i0 + tid, u = i >> LG, v = i & (G - 1);
    const int c = s_c[i];
    acc[0] += (unsigned)c;
    acc[1] += (unsigned)(c * c);
    acc[5] += c < 16;
    acc[6] += c > 239;
    const bool right = v < G - 1, below = u < G - 1;
    const int cr = right ? s_c[i + 1] : c, cb = below ? s_c[i + G] : c;           // a difference of 0 at the last column, row
    acc[3] += (unsigned)((cr - c) * (cr - c));
    acc[4] += (unsigned)((cb - c) * (cb - c));
    if (right && below && u >= 1 && v >= 1) {
      const int l = 4 * c - s_c[i - G] - cb - s_c[i - 1] - cr;                     // |l| <= 1020
      acc[2] += (unsigned)(l * l);
    }
  }

  // phase 3: the sums of the workgroup
#pragma unroll
  for (int k = 0; k < FQ_SUMS; ++k) {
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) acc[k] += __shfl_xor(acc[k], m, 64);
  }
  if ((tid & 63) == 0) {
#pragma unroll
    for (int k = 0; k < FQ_SUMS; ++k) s_part[tid >> 6][k] = acc[k];
  }
  __syncthreads();
  if (tid == 0) {
    FqOut r;
    r.v[0] = G;
#pragma unroll
    for (int k = 0; k < FQ_SUMS; ++k) {
      long long s = 0;
#pragma unroll
      for (int q = 0; q < FQ_THREADS / 64; ++q) s += (long long)s_part[q][k];
      r.v[1 + k] = s;
    }
    *dst = r;
  }
}

int launch_face_quality(const unsigned char* frames, int nframes, int H, int W, const int* boxes5, int n, int grid,
                        int64_t* out8, hipStream_t s) {
  GCV_REQUIRE(grid == 16 || grid == 32 || grid == 64, "face quality: grid is 16, 32 or 64");
  GCV_REQUIRE(nframes > 0 && H > 0 && W > 0, "face quality: bad geometry");
  GCV_REQUIRE((int64_t)H * W <= ((int64_t)1 << 30), "face quality: frames of more than 2^30 pixels");   // a cell's sum: 32 bits
  GCV_REQUIRE(n >= 0, "face quality: negative box count");
  if (n == 0) return 0;
  long long* out = reinterpret_cast<long long*>(out8);
  if (grid == 16)
    hipLaunchKernelGGL(face_quality_kernel<16>, dim3((unsigned)n), dim3(FQ_THREADS), 0, s, frames, nframes, H, W, boxes5, out);
  else if (grid == 32)
    hipLaunchKernelGGL(face_quality_kernel<32>, dim3((unsigned)n), dim3(FQ_THREADS), 0, s, frames, nframes, H, W, boxes5, out);
  else
    hipLaunchKernelGGL(face_quality_kernel<64>, dim3((unsigned)n), dim3(FQ_THREADS), 0, s, frames, nframes, H, W, boxes5, out);
  GCV_CHECK_HIP(hipGetLastError());
  return 0;
}

}  // namespace gcv
