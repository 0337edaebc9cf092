// The way back of face.hip: draw each face's evidence map (Grad-CAM, cam.hip / cam_bwd.hip) over the face box of the
// source frame as a colour heat overlay, all boxes of a clip in one launch (gcv_cam_overlay, include/genconvit_hip.h).
//
// One pass over the frames: every thread owns OV_CHUNKS x 4 whole pixels (12 bytes each: one dwordx3 load and store,
// consecutive lanes on consecutive 12 bytes), reads them once, applies the boxes that cover them in row order in
// registers and writes them once.  A pixel is read and written by its owner alone, so overlapping boxes need no atomics
// and out == frames is safe.  Why 12 bytes: a pixel is 3 bytes and a row 3 W, so 16-byte pieces start in the middle of a
// pixel (6 map samples for 5 1/3 pixels, the shared ones sampled twice) and need 16-byte aligned tensors; 12 bytes hold
// 4 whole pixels and need 4-byte alignment only.  The tensor is walked as one flat run of pixels, so odd W, rows that end
// inside a piece and frames that end inside a piece are the ordinary case: a piece's pixels carry their own (f, y, x).
// Tensors that are not 4-byte aligned, and the last partial piece, go byte by byte.
//
// Which boxes: a block covers 4096 consecutive pixels (a few rows of one frame as a rule).  Its threads test 256 boxes at
// a time against that range, the four wave ballots go through LDS, and every thread then walks the set bits in row
// order — block-uniform, so box fields are scalar loads and a block that no box touches is a plain copy.
//
// The arithmetic is fixed by the header so that tests/overlayutil.py can restate it bit for bit: integer sample
// positions, one fp32 rounding per multiply and add (fp contraction is off for this TU), round-half-even conversions,
// integer blend.
#pragma clang fp contract(off)
#include <cstdint>

#include "common.h"

namespace gcv {

constexpr int OV_THREADS = 256;   // 4 waves: one ballot word each
constexpr int OV_CHUNKS = 4;      // 12-byte pieces per thread, all loaded before the first is used
constexpr unsigned OV_BLOCK_PX = OV_THREADS * OV_CHUNKS * 4;

struct alignas(4) OvPiece { uint32_t w[3]; };   // 4 RGB pixels

struct OvCoef { int i0, i1; float l; };         // bilinear tap pair and weight of the second tap

// destination index j of a box side of s pixels over m map cells: F.interpolate(align_corners=False)'s source position
// ((2j + 1) m - s) / 2s, clamped at 0, split into cell and remainder in integers.  The quotient comes from one fp32
// product with inv_d = 1 / float(2s) and one correction step instead of an integer division: num < 2^25 and num / 2s < 224,
// so the three roundings (num, inv_d, the product) move the estimate by less than 224 * 3 * 2^-24 and its floor is within
// one of the quotient; the step makes it exact.
__device__ __forceinline__ OvCoef ov_coef(int j, int m, int s, float inv_d) {
  const int num = max((2 * j + 1) * m - s, 0), d = 2 * s;
  int q = (int)((float)num * inv_d);
  int r = num - q * d;
  if (r < 0) { q -= 1; r += d; }
  if (r >= d) { q += 1; r -= d; }
  OvCoef c;
  c.i0 = q;
  c.i1 = min(q + 1, m - 1);
  c.l = (float)r / (float)d;
  return c;
}

template <bool VEC>
__global__ void __launch_bounds__(OV_THREADS) cam_overlay_kernel(const unsigned char* frames, int nframes, int H, int W,
                                                                 const int* __restrict__ boxes, int n,
                                                                 const float* __restrict__ maps, int mh, int mw,
                                                                 const unsigned char* __restrict__ lut, float a256,
                                                                 int weighted, unsigned char* out) {
  __shared__ uint32_t s_lut[256];                      // r | g << 8 | b << 16
  __shared__ unsigned long long s_mask[OV_THREADS / 64];
  const int tid = threadIdx.x;
  const unsigned HW = (unsigned)H * (unsigned)W, P = (unsigned)nframes * HW;
  const unsigned blk0 = blockIdx.x * OV_BLOCK_PX, blk1 = min(blk0 + OV_BLOCK_PX, P);

  uint32_t w[OV_CHUNKS][3];
  int np[OV_CHUNKS];                                   // pixels of the piece that exist (0 past the end)
#pragma unroll
  for (int k = 0; k < OV_CHUNKS; ++k) {
    const unsigned p = blk0 + (unsigned)(k * OV_THREADS + tid) * 4u;
    np[k] = p < P ? (int)min(4u, P - p) : 0;
    const unsigned char* src = frames + (size_t)p * 3;
    if (VEC && np[k] == 4) {
      const OvPiece v = *reinterpret_cast<const OvPiece*>(src);
      w[k][0] = v.w[0]; w[k][1] = v.w[1]; w[k][2] = v.w[2];
    } else {
      w[k][0] = w[k][1] = w[k][2] = 0;
#pragma unroll
      for (int i = 0; i < 12; ++i)
        if (i < 3 * np[k]) w[k][i >> 2] |= (uint32_t)src[i] << (8 * (i & 3));
    }
  }

  unsigned dirty = 0;                                  // pieces a box changed
  if (n > 0) {
    s_lut[tid] = (uint32_t)lut[3 * tid] | (uint32_t)lut[3 * tid + 1] << 8 | (uint32_t)lut[3 * tid + 2] << 16;
    const unsigned f0 = blk0 / HW, f1 = (blk1 - 1) / HW;
    const unsigned y0 = (blk0 - f0 * HW) / (unsigned)W, y1 = (blk1 - 1 - f1 * HW) / (unsigned)W;
    bool have_pos = false;
    int pf[OV_CHUNKS], py[OV_CHUNKS], px[OV_CHUNKS];   // (frame, row, column) of each piece's first pixel
    for (int base = 0; base < n; base += OV_THREADS) {
      bool cand = false;
      if (base + tid < n) {
        const int* b = boxes + 5 * (size_t)(base + tid);
        const int f = b[0], top = b[1], right = b[2], bottom = b[3], left = b[4];
        const bool valid = f >= 0 && f < nframes && top >= 0 && left >= 0 && bottom <= H && right <= W && top < bottom &&
                           left < right;               // a box outside its frame draws nothing
        cand = valid && (unsigned)f >= f0 && (unsigned)f <= f1 &&
               (f0 != f1 || ((unsigned)bottom > y0 && (unsigned)top <= y1));
      }
      const unsigned long long m = __ballot(cand);
      if ((tid & 63) == 0) s_mask[tid >> 6] = m;
      __syncthreads();
#pragma unroll 1
      for (int wv = 0; wv < OV_THREADS / 64; ++wv) {
        const unsigned long long sm = s_mask[wv];
        unsigned long long mm = (unsigned long long)__builtin_amdgcn_readfirstlane((int)(sm >> 32)) << 32 |
                                (unsigned)__builtin_amdgcn_readfirstlane((int)sm);
        while (mm) {
          const int bi = base + 64 * wv + __builtin_ctzll(mm);
          mm &= mm - 1;
          if (!have_pos) {
            have_pos = true;
#pragma unroll
            for (int k = 0; k < OV_CHUNKS; ++k) {
              const unsigned p = blk0 + (unsigned)(k * OV_THREADS + tid) * 4u;
              const unsigned f = p / HW, r = p - f * HW, y = r / (unsigned)W;
              pf[k] = (int)f; py[k] = (int)y; px[k] = (int)(r - y * (unsigned)W);
            }
          }
          const int* b = boxes + 5 * (size_t)bi;
          const int bf = b[0], top = b[1], right = b[2], bottom = b[3], left = b[4];
          const int bh = bottom - top, bw = right - left;
          const float* mp = maps + (size_t)bi * mh * mw;
          const float inv_dy = 1.0f / (float)(2 * bh), inv_dx = 1.0f / (float)(2 * bw);
          // One copy of the sampling code for the thread's pieces: a rolled loop that works on piece 0 and then rotates
          // the pieces' registers by one (static indices, so they stay registers).  Unrolled it is four times the code
          // and measured the same time.
#pragma unroll 1
          for (int k = 0; k < OV_CHUNKS; ++k) {
            int f = pf[0], y = py[0], x = px[0];
            bool in[4], any = false;
            int jy[4], jx[4];
#pragma unroll
            for (int q = 0; q < 4; ++q) {
              in[q] = q < np[0] && f == bf && y >= top && y < bottom && x >= left && x < right;
              any |= in[q];
              jy[q] = min(max(y - top, 0), bh - 1);    // pixels outside sample a cell of the map all the same and
              jx[q] = min(max(x - left, 0), bw - 1);   // are blended with weight 0: the piece's 16 taps load together
              if (++x == W) { x = 0; if (++y == H) { y = 0; ++f; } }
            }
            if (any) {
              dirty |= 1u << k;
              OvCoef cy[4];                              // rows first: a row ends inside few pieces, and the branch
              cy[0] = ov_coef(jy[0], mh, bh, inv_dy);    // stays out of the loop whose loads are to issue together
#pragma unroll
              for (int q = 1; q < 4; ++q) {
                cy[q] = cy[q - 1];
                if (jy[q] != jy[q - 1]) cy[q] = ov_coef(jy[q], mh, bh, inv_dy);
              }
              const uint32_t pix[4] = {w[0][0] & 0xFFFFFFu, (w[0][0] >> 24 | w[0][1] << 8) & 0xFFFFFFu,
                                       (w[0][1] >> 16 | w[0][2] << 16) & 0xFFFFFFu, w[0][2] >> 8};
              uint32_t o[4];
              float lx[4], m00[4], m01[4], m10[4], m11[4];
#pragma unroll
              for (int q = 0; q < 4; ++q) {              // the piece's 16 taps, issued together
                const OvCoef cx = ov_coef(jx[q], mw, bw, inv_dx);
                const unsigned r0 = (unsigned)(cy[q].i0 * mw), r1 = (unsigned)(cy[q].i1 * mw);
                lx[q] = cx.l;
                m00[q] = mp[r0 + (unsigned)cx.i0]; m01[q] = mp[r0 + (unsigned)cx.i1];
                m10[q] = mp[r1 + (unsigned)cx.i0]; m11[q] = mp[r1 + (unsigned)cx.i1];
              }
#pragma unroll
              for (int q = 0; q < 4; ++q) {
                const float ax = 1.0f - lx[q], ay = 1.0f - cy[q].l;
                const float t0 = m00[q] * ax + m01[q] * lx[q], t1 = m10[q] * ax + m11[q] * lx[q];
                float v = t0 * ay + t1 * cy[q].l;
                v = fminf(fmaxf(v, 0.0f), 1.0f);         // a NaN becomes 0
                const int kk = __float2int_rn(v * 255.0f);
                const uint32_t a8 = in[q] ? (uint32_t)min(max(__float2int_rn(weighted ? a256 * v : a256), 0), 256) : 0u;
                const uint32_t col = s_lut[kk], ia = 256u - a8;
                // (frame_c (256 - a8) + lut_c a8 + 128) >> 8 for R and B in one word, G in another: a channel's sum is at
                // most 255 * 256 + 128 and stays inside its 16 bits; a8 = 0 gives the pixel back
                const uint32_t rb = ((pix[q] & 0xFF00FFu) * ia + (col & 0xFF00FFu) * a8 + 0x800080u) >> 8 & 0xFF00FFu;
                const uint32_t g = ((pix[q] & 0x00FF00u) * ia + (col & 0x00FF00u) * a8 + 0x008000u) >> 8 & 0x00FF00u;
                o[q] = rb | g;
              }
              w[0][0] = o[0] | o[1] << 24;
              w[0][1] = o[1] >> 8 | o[2] << 16;
              w[0][2] = o[2] >> 16 | o[3] << 8;
            }
#pragma unroll
            for (int i = 0; i < OV_CHUNKS - 1; ++i) {  // rotate: piece i + 1 becomes piece i, piece 0 the last
#pragma unroll
              for (int j = 0; j < 3; ++j) { const uint32_t t = w[i][j]; w[i][j] = w[i + 1][j]; w[i + 1][j] = t; }
              int t;
              t = np[i]; np[i] = np[i + 1]; np[i + 1] = t;
              t = pf[i]; pf[i] = pf[i + 1]; pf[i + 1] = t;
              t = py[i]; py[i] = py[i + 1]; py[i + 1] = t;
              t = px[i]; px[i] = px[i + 1]; px[i + 1] = t;
            }
          }
        }
      }
      __syncthreads();
    }
  }

  const bool inplace = out == frames;                  // in place, untouched pieces are already there
#pragma unroll
  for (int k = 0; k < OV_CHUNKS; ++k) {
    if (np[k] == 0 || (inplace && !(dirty >> k & 1u))) continue;
    const unsigned p = blk0 + (unsigned)(k * OV_THREADS + tid) * 4u;
    unsigned char* dst = out + (size_t)p * 3;
    if (VEC && np[k] == 4) {
      OvPiece v;
      v.w[0] = w[k][0]; v.w[1] = w[k][1]; v.w[2] = w[k][2];
      *reinterpret_cast<OvPiece*>(dst) = v;
    } else {
#pragma unroll
      for (int i = 0; i < 12; ++i)
        if (i < 3 * np[k]) dst[i] = (unsigned char)(w[k][i >> 2] >> (8 * (i & 3)));
    }
  }
}

int launch_cam_overlay(const unsigned char* frames, int nframes, int H, int W, const int* boxes, int n, const float* maps,
                       int mh, int mw, const unsigned char* lut, float alpha, int weighted, unsigned char* out,
                       hipStream_t s) {
  GCV_REQUIRE(nframes > 0 && H > 0 && W > 0 && H <= 65536 && W <= 65536, "cam overlay: bad geometry");
  const int64_t pixels = (int64_t)nframes * H * W;
  GCV_REQUIRE(pixels < ((int64_t)1 << 31), "cam overlay: too many pixels for one launch");
  GCV_REQUIRE(n >= 0, "cam overlay: negative box count");
  GCV_REQUIRE(n == 0 || (mh >= 1 && mh <= 224 && mw >= 1 && mw <= 224), "cam overlay: maps are 1 ... 224 cells a side");
  GCV_REQUIRE(alpha >= 0.0f && alpha <= 1.0f, "cam overlay: alpha outside [0, 1]");
  if (n == 0 && out == frames) return 0;
  const unsigned grid = (unsigned)((pixels + OV_BLOCK_PX - 1) / OV_BLOCK_PX);
  const float a256 = alpha * 256.0f;
  if ((((uintptr_t)frames | (uintptr_t)out) & 3u) == 0)
    hipLaunchKernelGGL(cam_overlay_kernel<true>, dim3(grid), dim3(OV_THREADS), 0, s, frames, nframes, H, W, boxes, n, maps,
                       mh, mw, lut, a256, weighted, out);
  else
    hipLaunchKernelGGL(cam_overlay_kernel<false>, dim3(grid), dim3(OV_THREADS), 0, s, frames, nframes, H, W, boxes, n, maps,
                       mh, mw, lut, a256, weighted, out);
  GCV_CHECK_HIP(hipGetLastError());
  return 0;
}

}  // namespace gcv
