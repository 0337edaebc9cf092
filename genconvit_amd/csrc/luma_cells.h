// The mean-luma cells of a face box, shared by follow.hip (gcv_track_match), quality.hip (gcv_face_quality) and persons.hip
// (gcv_face_signature): include/genconvit_hip.h fixes the arithmetic at gcv_track_match.
#pragma once
#include <cstdint>

namespace gcv {

struct TmBox { int f, top, right, bottom, left; };

__device__ __forceinline__ bool tm_box_ok(const TmBox& b, int nframes, int H, int W, int G) {
  return b.f >= 0 && b.f < nframes && b.top >= 0 && b.left >= 0 && b.bottom <= H && b.right <= W && b.top <= b.bottom &&
         b.left <= b.right && b.bottom - b.top >= G && b.right - b.left >= G;
}

// (sum of Y over rows [y0, y1) x columns [x0, x1) + cnt / 2) / cnt with Y = (77 R + 150 G + 29 B + 128) >> 8
__device__ __forceinline__ unsigned tm_cell(const unsigned char* __restrict__ frame, int64_t rs, int y0, int y1, int x0,
                                            int x1) {
  unsigned sum = 0;
  for (int y = y0; y < y1; ++y) {
    const unsigned char* p = frame + (int64_t)y * rs + (int64_t)x0 * 3;
    for (int x = x0; x < x1; ++x, p += 3) sum += (77u * p[0] + 150u * p[1] + 29u * p[2] + 128u) >> 8;
  }
  const unsigned cnt = (unsigned)(y1 - y0) * (unsigned)(x1 - x0);
  return (sum + cnt / 2u) / cnt;
}

// tm_cell of the same rectangle, and beside it the rectangle's sums of Cb = (32896 - 43 R - 85 G + 128 B) >> 8 and
// Cr = (32896 + 128 R - 107 G - 21 B) >> 8 (both 1 ... 256, so unsigned arithmetic is exact) for persons.hip
// (gcv_face_signature): the caller adds the sums of the rectangles that make up a chroma cell and divides once.
__device__ __forceinline__ unsigned tm_cell_ycc(const unsigned char* __restrict__ frame, int64_t rs, int y0, int y1, int x0,
                                                int x1, unsigned& cb_sum, unsigned& cr_sum) {
  unsigned sum = 0, cb = 0, cr = 0;
  for (int y = y0; y < y1; ++y) {
    const unsigned char* p = frame + (int64_t)y * rs + (int64_t)x0 * 3;
    for (int x = x0; x < x1; ++x, p += 3) {
      const unsigned r = p[0], g = p[1], b = p[2];
      sum += (77u * r + 150u * g + 29u * b + 128u) >> 8;
      cb += (32896u - 43u * r - 85u * g + 128u * b) >> 8;
      cr += (32896u + 128u * r - 107u * g - 21u * b) >> 8;
    }
  }
  const unsigned cnt = (unsigned)(y1 - y0) * (unsigned)(x1 - x0);
  cb_sum = cb;
  cr_sum = cr;
  return (sum + cnt / 2u) / cnt;
}

}  // namespace gcv
