// The way back of the scan: draw its result onto the frames it was run on — a box outline per crop row in the colour of
// its score, a small number tab in the box's corner, a timeline strip along the bottom edge with a cursor at the frame's
// own place (gcv_scan_annotate, include/genconvit_hip.h).  All marks of a group of frames and the strip in one launch.
//
// The walk over the frames is overlay.hip's: every thread owns AN_CHUNKS x 4 whole pixels (12 bytes each: one dwordx3
// load and store, consecutive lanes on consecutive 12 bytes), reads them once, applies the marks that cover them in row
// order and then the strip, all in registers, and writes them once.  A pixel is read and written by its owner alone, so
// overlapping marks need no atomics and out == frames is safe.  The tensor is one flat run of pixels: rows and frames
// that end inside a piece are the ordinary case, a piece's pixels carry their own (f, y, x).  Tensors that are not
// 4-byte aligned, and the last partial piece, go byte by byte.
//
// Which marks: a block covers 4096 consecutive pixels.  Its threads test 256 marks at a time against that range, the
// four wave ballots go through LDS, and every thread then walks the set bits in row order — block-uniform, so a mark's
// fields are scalar loads and its label bitmap is built once per block in scalar registers.  A block that no mark and
// no strip row touches is a plain copy, and writes nothing when the call is in place.
//
// The piece load/store and the ballot cull are restated here rather than shared with overlay.hip: that kernel's code
// stays byte for byte what its timing record was measured on.
//
// The arithmetic is all-integer and fixed by the header, so that tests/annotateutil.py restates it bit for bit.
#include <cstdint>

#include "common.h"

namespace gcv {

constexpr int AN_THREADS = 256;   // 4 waves: one ballot word each
constexpr int AN_CHUNKS = 4;      // 12-byte pieces per thread, all loaded before the first is used
constexpr unsigned AN_BLOCK_PX = AN_THREADS * AN_CHUNKS * 4;

struct alignas(4) AnPiece { uint32_t w[3]; };   // 4 RGB pixels

// the 3 x 5 digits, rows top to bottom, bit (row * 3 + column) set where there is ink
constexpr uint16_t an_glyph(const char (&s)[16]) {
  uint16_t v = 0;
  for (int i = 0; i < 15; ++i) v |= (uint16_t)((s[i] == '1') << i);
  return v;
}
__constant__ const uint16_t AN_FONT[10] = {
    an_glyph("111101101101111"), an_glyph("010110010010111"), an_glyph("111001111100111"), an_glyph("111001111001111"),
    an_glyph("101101111001001"), an_glyph("111100111001111"), an_glyph("111100111101111"), an_glyph("111001001001001"),
    an_glyph("111101111101111"), an_glyph("111101111001111")};

__device__ __forceinline__ void an_unpack(const uint32_t (&w)[3], uint32_t (&pix)[4]) {
  pix[0] = w[0] & 0xFFFFFFu;
  pix[1] = (w[0] >> 24 | w[1] << 8) & 0xFFFFFFu;
  pix[2] = (w[1] >> 16 | w[2] << 16) & 0xFFFFFFu;
  pix[3] = w[2] >> 8;
}

__device__ __forceinline__ void an_pack(uint32_t (&w)[3], const uint32_t (&pix)[4]) {
  w[0] = pix[0] | pix[1] << 24;
  w[1] = pix[1] >> 8 | pix[2] << 16;
  w[2] = pix[2] >> 16 | pix[3] << 8;
}

template <bool VEC>
__global__ void __launch_bounds__(AN_THREADS) scan_annotate_kernel(const unsigned char* frames, int nframes, int H, int W,
                                                                   const int* __restrict__ frame_no,
                                                                   const int* __restrict__ marks, int n,
                                                                   const unsigned* __restrict__ timeline, int lanes, int T,
                                                                   int strip, unsigned char* out) {
  __shared__ unsigned long long s_mask[AN_THREADS / 64];
  const int tid = threadIdx.x;
  const unsigned HW = (unsigned)H * (unsigned)W, P = (unsigned)nframes * HW;
  const unsigned blk0 = blockIdx.x * AN_BLOCK_PX, blk1 = min(blk0 + AN_BLOCK_PX, P);

  uint32_t w[AN_CHUNKS][3];
  int np[AN_CHUNKS];                                   // pixels of the piece that exist (0 past the end)
#pragma unroll
  for (int k = 0; k < AN_CHUNKS; ++k) {
    const unsigned p = blk0 + (unsigned)(k * AN_THREADS + tid) * 4u;
    np[k] = p < P ? (int)min(4u, P - p) : 0;
    const unsigned char* src = frames + (size_t)p * 3;
    if (VEC && np[k] == 4) {
      const AnPiece v = *reinterpret_cast<const AnPiece*>(src);
      w[k][0] = v.w[0]; w[k][1] = v.w[1]; w[k][2] = v.w[2];
    } else {
      w[k][0] = w[k][1] = w[k][2] = 0;
#pragma unroll
      for (int i = 0; i < 12; ++i)
        if (i < 3 * np[k]) w[k][i >> 2] |= (uint32_t)src[i] << (8 * (i & 3));
    }
  }

  // the block's pixel range as frames and rows: what the marks and the strip are tested against
  const unsigned f0 = blk0 / HW, f1 = (blk1 - 1) / HW;
  const unsigned y0 = (blk0 - f0 * HW) / (unsigned)W, y1 = (blk1 - 1 - f1 * HW) / (unsigned)W;
  const bool in_strip = strip > 0 && (f0 != f1 || y1 >= (unsigned)(H - strip));   // a frame's end is its bottom row

  unsigned dirty = 0;                                  // pieces that something drew on
  bool have_pos = false;
  int pf[AN_CHUNKS], py[AN_CHUNKS], px[AN_CHUNKS];     // (frame, row, column) of each piece's first pixel
  auto positions = [&]() {
    have_pos = true;
#pragma unroll
    for (int k = 0; k < AN_CHUNKS; ++k) {
      const unsigned p = blk0 + (unsigned)(k * AN_THREADS + tid) * 4u;
      const unsigned f = p / HW, r = p - f * HW, y = r / (unsigned)W;
      pf[k] = (int)f; py[k] = (int)y; px[k] = (int)(r - y * (unsigned)W);
    }
  };

  for (int base = 0; base < n; base += AN_THREADS) {
    bool cand = false;
    if (base + tid < n) {
      const int* m = marks + 8 * (size_t)(base + tid);
      const int f = m[0], top = m[1], right = m[2], bottom = m[3], left = m[4], thick = m[6], label = m[7];
      const bool valid = f >= 0 && f < nframes && top >= 0 && left >= 0 && bottom <= H && right <= W && top < bottom &&
                         left < right && thick >= 1 && thick <= 16 && label >= -1 && label <= 999;
      cand = valid && (unsigned)f >= f0 && (unsigned)f <= f1 &&
             (f0 != f1 || ((unsigned)bottom > y0 && (unsigned)top <= y1));
    }
    const unsigned long long bal = __ballot(cand);
    if ((tid & 63) == 0) s_mask[tid >> 6] = bal;
    __syncthreads();
#pragma unroll 1
    for (int wv = 0; wv < AN_THREADS / 64; ++wv) {
      const unsigned long long sm = s_mask[wv];
      unsigned long long mm = (unsigned long long)__builtin_amdgcn_readfirstlane((int)(sm >> 32)) << 32 |
                              (unsigned)__builtin_amdgcn_readfirstlane((int)sm);
      while (mm) {
        const int bi = base + 64 * wv + __builtin_ctzll(mm);
        mm &= mm - 1;
        if (!have_pos) positions();
        const int* m = marks + 8 * (size_t)bi;
        const int mf = m[0], top = m[1], right = m[2], bottom = m[3], left = m[4], thick = m[6], label = m[7];
        const uint32_t colour = (uint32_t)m[5] & 0xFFFFFFu;
        const uint32_t luma = (77u * (colour & 255u) + 150u * (colour >> 8 & 255u) + 29u * (colour >> 16)) >> 8;
        const uint32_t ink = luma >= 128u ? 0u : 0xFFFFFFu;
        // a / thick for 0 <= a <= 255 as (a rcp) >> 16 with rcp = ceil(2^16 / thick): rcp thick - 2^16 < thick <= 16, so
        // a rcp exceeds a 2^16 / thick by less than 255 * 16 / thick < 2^16 / thick, too little to reach the next quotient
        const unsigned rcp = (65536u + (unsigned)thick - 1u) / (unsigned)thick;
        // the label as one bitmap: bit (cy - 1) * 12 + (cx - 1) is ink, 5 rows of up to 3 digits 4 cells apart
        const int nd = label >= 100 ? 3 : label >= 10 ? 2 : 1;
        const int tabw = label >= 0 ? 4 * nd + 1 : 0;
        unsigned long long bits = 0;
        if (label >= 0) {
          const int d100 = label / 100, d10 = label / 10 % 10, d1 = label % 10;
          const int digit[3] = {nd == 3 ? d100 : nd == 2 ? d10 : d1, nd == 3 ? d10 : d1, d1};   // most significant first
#pragma unroll
          for (int k = 0; k < 3; ++k) {
            if (k >= nd) continue;
            const unsigned long long g = AN_FONT[digit[k]];
#pragma unroll
            for (int r = 0; r < 5; ++r) bits |= (g >> (3 * r) & 7ull) << (12 * r + 4 * k);
          }
        }
#pragma unroll
        for (int k = 0; k < AN_CHUNKS; ++k) {
          int f = pf[k], y = py[k], x = px[k];
          bool draw[4], any = false;
          uint32_t val[4];
#pragma unroll
          for (int q = 0; q < 4; ++q) {
            const int dy = y - top, dx = x - left;
            const bool in = q < np[k] && f == mf && y >= top && y < bottom && x >= left && x < right;
            const bool edge = dy < thick || bottom - 1 - y < thick || dx < thick || right - 1 - x < thick;
            // past 255 pixels from the corner a pixel is in no tab (7 * 16 rows, 13 * 16 columns at the most)
            const int cy = (int)((unsigned)min(max(dy, 0), 255) * rcp >> 16);
            const int cx = (int)((unsigned)min(max(dx, 0), 255) * rcp >> 16);
            const bool tab = cy < 7 && cx < tabw;
            const bool on = tab && cy >= 1 && cy <= 5 && cx >= 1 && (bits >> (((cy - 1) * 12 + (cx - 1)) & 63) & 1ull);
            draw[q] = in && (edge || tab);
            val[q] = on ? ink : colour;
            any |= draw[q];
            if (++x == W) { x = 0; if (++y == H) { y = 0; ++f; } }
          }
          if (any) {
            dirty |= 1u << k;
            uint32_t pix[4];
            an_unpack(w[k], pix);
#pragma unroll
            for (int q = 0; q < 4; ++q) pix[q] = draw[q] ? val[q] : pix[q];
            an_pack(w[k], pix);
          }
        }
      }
    }
    __syncthreads();
  }

  if (in_strip) {                                      // over the marks
    if (!have_pos) positions();
    const int ys = H - strip;
#pragma unroll
    for (int k = 0; k < AN_CHUNKS; ++k) {
      int f = pf[k], y = py[k], x = px[k];
      bool draw[4], any = false;
      uint32_t val[4];
      int at_f = -1, at_y = -1, x0 = 0, x1 = 0;
      unsigned row = 0;
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        draw[q] = q < np[k] && y >= ys;
        val[q] = 0;
        if (draw[q]) {
          any = true;
          if (y != at_y) {                             // the lane of this row
            at_y = y;
            row = ((unsigned)(y - ys) * (unsigned)lanes / (unsigned)strip) * (unsigned)T;
          }
          if (f != at_f) {                             // the cursor of this frame: c W < T W < 2^31
            at_f = f;
            const int c = frame_no[f];
            x0 = x1 = 0;
            if (c >= 0 && c < T) {
              x0 = (int)((unsigned)c * (unsigned)W / (unsigned)T);
              x1 = max(x0 + 1, (int)((unsigned)(c + 1) * (unsigned)W / (unsigned)T));
            }
          }
          const unsigned t = (unsigned)x * (unsigned)T / (unsigned)W;
          val[q] = x >= x0 && x < x1 ? 0xFFFFFFu : timeline[row + t] & 0xFFFFFFu;
        }
        if (++x == W) { x = 0; if (++y == H) { y = 0; ++f; } }
      }
      if (any) {
        dirty |= 1u << k;
        uint32_t pix[4];
        an_unpack(w[k], pix);
#pragma unroll
        for (int q = 0; q < 4; ++q) pix[q] = draw[q] ? val[q] : pix[q];
        an_pack(w[k], pix);
      }
    }
  }

  const bool inplace = out == frames;                  // in place, untouched pieces are already there
#pragma unroll
  for (int k = 0; k < AN_CHUNKS; ++k) {
    if (np[k] == 0 || (inplace && !(dirty >> k & 1u))) continue;
    const unsigned p = blk0 + (unsigned)(k * AN_THREADS + tid) * 4u;
    unsigned char* dst = out + (size_t)p * 3;
    if (VEC && np[k] == 4) {
      AnPiece v;
      v.w[0] = w[k][0]; v.w[1] = w[k][1]; v.w[2] = w[k][2];
      *reinterpret_cast<AnPiece*>(dst) = v;
    } else {
#pragma unroll
      for (int i = 0; i < 12; ++i)
        if (i < 3 * np[k]) dst[i] = (unsigned char)(w[k][i >> 2] >> (8 * (i & 3)));
    }
  }
}

int launch_scan_annotate(const unsigned char* frames, int nframes, int H, int W, const int* frame_no, const int* marks,
                         int n, const unsigned* timeline, int lanes, int T, int strip, unsigned char* out, hipStream_t s) {
  GCV_REQUIRE(nframes > 0 && H > 0 && W > 0 && H <= 65536 && W <= 65536, "scan annotate: bad geometry");
  const int64_t pixels = (int64_t)nframes * H * W;
  GCV_REQUIRE(pixels < ((int64_t)1 << 31), "scan annotate: too many pixels for one launch");
  GCV_REQUIRE(n >= 0 && strip >= 0, "scan annotate: negative mark count or strip height");
  if (strip > 0) {
    GCV_REQUIRE(lanes >= 1 && lanes <= 8 && lanes <= strip && strip <= H, "scan annotate: 1 <= lanes <= 8, lanes <= strip <= H");
    GCV_REQUIRE(T >= 1 && (int64_t)T * W < ((int64_t)1 << 31), "scan annotate: T >= 1 and T W < 2^31");
  }
  if (n == 0 && strip == 0 && out == frames) return 0;
  const unsigned grid = (unsigned)((pixels + AN_BLOCK_PX - 1) / AN_BLOCK_PX);
  if ((((uintptr_t)frames | (uintptr_t)out) & 3u) == 0)
    hipLaunchKernelGGL(scan_annotate_kernel<true>, dim3(grid), dim3(AN_THREADS), 0, s, frames, nframes, H, W, frame_no, marks,
                       n, timeline, lanes, T, strip, out);
  else
    hipLaunchKernelGGL(scan_annotate_kernel<false>, dim3(grid), dim3(AN_THREADS), 0, s, frames, nframes, H, W, frame_no,
                       marks, n, timeline, lanes, T, strip, out);
  GCV_CHECK_HIP(hipGetLastError());
  return 0;
}

}  // namespace gcv
