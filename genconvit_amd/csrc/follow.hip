// Follow a face between two detector frames by integer block matching (gcv_track_match, include/genconvit_hip.h, which
// fixes the arithmetic; tests/followutil.py restates it bit for bit).  The detector of a whole-video scan runs on every
// k-th frame; in a skipped frame the face is searched around the interpolated box, with the two detected faces around the
// gap as templates.  Everything is compared on a G x G grid of mean-luma cells, each box at its own size, so a face that
// grows or shrinks across the gap is matched at a normalised scale and the displacements count cells, not pixels.
//
// One workgroup per job, three phases:
//   1. the window cells V (only those a valid candidate can use: they lie inside the frame) and the templates A, B as
//      bytes in LDS.  One thread = one cell; consecutive lanes take consecutive cells of a cell row, so a wave's reads
//      of one pixel row are one contiguous run of RGB bytes.
//   2. the valid candidates (a rectangle of displacements: validity is separable in y and x and monotone in each) are
//      dealt over the lanes, consecutive dx on consecutive lanes.  A lane walks the G rows of its candidate four cells
//      at a time: the template dwords sit at a wave-uniform LDS address (broadcast), the window bytes start at any byte
//      offset, so a lane reads the aligned dwords around them and shifts with v_alignbyte_b32; two v_sad_u8 add the four
//      |A - V| and |B - V|.  The weights multiply the two sums once, at the end.
//   3. min of the packed key cost << 32 | d2 << 16 | (dy + R) << 8 | (dx + R) across each wave by shuffles, across the
//      waves through LDS; one lane writes the 16 bytes.
// No atomics, no scratch, nothing allocated or synchronised.  The jobs of one gap recompute the same two templates: at
// most 2 of the (G + 2R)^2 / G^2 + 2 cell grids a job builds, accepted for one launch with no pass in front of it.
#include <cstdint>

#include "common.h"
#include "luma_cells.h"                                   // TmBox, tm_box_ok, tm_cell

namespace gcv {

constexpr int TM_THREADS = 256;
constexpr int TM_RMAX = 32;

struct alignas(4) TmOut { int v[4]; };

template <int G>
__global__ void __launch_bounds__(TM_THREADS) track_match_kernel(const unsigned char* __restrict__ frames, int nframes,
                                                                 int H, int W, const int* __restrict__ jobs, int R,
                                                                 int* __restrict__ out) {
  constexpr int LG = G == 16 ? 4 : (G == 32 ? 5 : 6);
  constexpr int NE = G + 2 * TM_RMAX + 1;                  // edges of the window cells u = -R ... G + R
  // window cell (u, v) at byte (u + R) * ws + (v + R); ws is a multiple of 4 with 4 spare bytes, G + 68 at the most
  __shared__ __attribute__((aligned(16))) unsigned char s_win[(G + 2 * TM_RMAX) * (G + 2 * TM_RMAX + 4)];
  __shared__ __attribute__((aligned(16))) unsigned char s_tpl[2][G * G];
  __shared__ int s_ey[NE], s_ex[NE], s_ty[2][G + 1], s_tx[2][G + 1];
  __shared__ unsigned long long s_key[TM_THREADS / 64];
  __shared__ unsigned s_cost0;

  const int tid = threadIdx.x;
  const int* j = jobs + 17 * (size_t)blockIdx.x;
  const TmBox p = {j[0], j[1], j[2], j[3], j[4]};
  const TmBox a = {j[5], j[6], j[7], j[8], j[9]}, b = {j[11], j[12], j[13], j[14], j[15]};
  const int wa = j[10], wb = j[16];
  TmOut* dst = reinterpret_cast<TmOut*>(out + 4 * (size_t)blockIdx.x);
  // a bad row (block-uniform): read nothing, write zeros
  if (!(tm_box_ok(p, nframes, H, W, G) && tm_box_ok(a, nframes, H, W, G) && tm_box_ok(b, nframes, H, W, G) &&
        wa >= 0 && wb >= 0 && (unsigned)wa + (unsigned)wb >= 1u && (unsigned)wa + (unsigned)wb <= 1024u)) {
    if (tid == 0) *dst = TmOut{{0, 0, 0, 0}};
    return;
  }
  const int h = p.bottom - p.top, w = p.right - p.left;

  // cell edges e(u) = floor(u * extent / G): the shift is a floor division for negative u as well
  for (int i = tid; i <= G + 2 * R; i += TM_THREADS) {
    s_ey[i] = (int)(((int64_t)(i - R) * h) >> LG);
    s_ex[i] = (int)(((int64_t)(i - R) * w) >> LG);
  }
  for (int i = tid; i < 2 * (G + 1); i += TM_THREADS) {
    const int t = i > G, u = t ? i - (G + 1) : i;
    s_ty[t][u] = (int)(((int64_t)u * (t ? b.bottom - b.top : a.bottom - a.top)) >> LG);
    s_tx[t][u] = (int)(((int64_t)u * (t ? b.right - b.left : a.right - a.left)) >> LG);
  }
  __syncthreads();

  // valid displacements: e is monotone, so they are the ranges around 0 in which the displaced box stays in the frame
  int dy_lo = 0, dy_hi = 0, dx_lo = 0, dx_hi = 0;
  while (dy_lo > -R && p.top + s_ey[dy_lo - 1 + R] >= 0) --dy_lo;
  while (dy_hi < R && p.bottom + s_ey[dy_hi + 1 + R] <= H) ++dy_hi;
  while (dx_lo > -R && p.left + s_ex[dx_lo - 1 + R] >= 0) --dx_lo;
  while (dx_hi < R && p.right + s_ex[dx_hi + 1 + R] <= W) ++dx_hi;
  const int ws = ((G + 2 * R + 3) & ~3) + 4;

  // phase 1: the window cells u in [dy_lo, dy_hi + G), v in [dx_lo, dx_hi + G) — together the displaced boxes of the valid
  // candidates, all inside the frame — and the two templates
  {
    const int64_t rs = (int64_t)W * 3;
    const int nxc = dx_hi - dx_lo + G, nwin = (dy_hi - dy_lo + G) * nxc;
    for (int i = tid; i < nwin + 2 * G * G; i += TM_THREADS) {
      if (i < nwin) {
        const int r = i / nxc, iu = r + dy_lo + R, iv = i - r * nxc + dx_lo + R;
        s_win[iu * ws + iv] = (unsigned char)tm_cell(frames + (int64_t)p.f * H * rs, rs, p.top + s_ey[iu],
                                                     p.top + s_ey[iu + 1], p.left + s_ex[iv], p.left + s_ex[iv + 1]);
      } else {
        const int k = i - nwin, t = k >> (2 * LG), u = (k >> LG) & (G - 1), v = k & (G - 1);
        const int f = t ? b.f : a.f, top = t ? b.top : a.top, left = t ? b.left : a.left;
        s_tpl[t][u * G + v] = (unsigned char)tm_cell(frames + (int64_t)f * H * rs, rs, top + s_ty[t][u], top + s_ty[t][u + 1],
                                                     left + s_tx[t][v], left + s_tx[t][v + 1]);
      }
    }
  }
  __syncthreads();

  // phase 2: candidates over the lanes
  unsigned long long best = ~0ull;
  {
    const int nx = dx_hi - dx_lo + 1, ncand = (dy_hi - dy_lo + 1) * nx;
    const uint32_t* ta = reinterpret_cast<const uint32_t*>(s_tpl[0]);
    const uint32_t* tb = reinterpret_cast<const uint32_t*>(s_tpl[1]);
    for (int c = tid; c < ncand; c += TM_THREADS) {
      const int cy = c / nx, dy = dy_lo + cy, dx = dx_lo + (c - cy * nx);
      const unsigned sh = (unsigned)(dx + R) & 3u;
      const uint32_t* wrow = reinterpret_cast<const uint32_t*>(s_win + (dy + R) * ws) + ((dx + R) >> 2);
      unsigned sa = 0, sb = 0;
#pragma unroll 1
      for (int u = 0; u < G; ++u, wrow += ws >> 2) {
        uint32_t lo = wrow[0];
#pragma unroll
        for (int q = 0; q < G / 4; ++q) {
          const uint32_t hi = wrow[q + 1];                 // past the last cell for q = G / 4 - 1: inside the row's spare
          const uint32_t v = __builtin_amdgcn_alignbyte(hi, lo, sh);      // bytes, and shifted out again
          sa = __builtin_amdgcn_sad_u8(ta[u * (G / 4) + q], v, sa);
          sb = __builtin_amdgcn_sad_u8(tb[u * (G / 4) + q], v, sb);
          lo = hi;
        }
      }
      const unsigned cost = (unsigned)wa * sa + (unsigned)wb * sb;       // <= 1024 * G * G * 255 < 2^31
      if (dy == 0 && dx == 0) s_cost0 = cost;
      const unsigned long long key = (unsigned long long)cost << 32 | (unsigned long long)(dy * dy + dx * dx) << 16 |
                                     (unsigned long long)(dy + R) << 8 | (unsigned long long)(dx + R);
      best = key < best ? key : best;
    }
  }

  // phase 3: the smallest key of the workgroup
#pragma unroll
  for (int m = 32; m >= 1; m >>= 1) {
    const unsigned long long o = __shfl_xor(best, m, 64);
    best = o < best ? o : best;
  }
  if ((tid & 63) == 0) s_key[tid >> 6] = best;
  __syncthreads();
  if (tid == 0) {
#pragma unroll
    for (int k = 1; k < TM_THREADS / 64; ++k) best = s_key[k] < best ? s_key[k] : best;
    const int dy = (int)(best >> 8 & 0xFFu), dx = (int)(best & 0xFFu);   // still offset by R: the index of the edge
    *dst = TmOut{{s_ey[dy], s_ex[dx], (int)(best >> 32), (int)s_cost0}};
  }
}

int launch_track_match(const unsigned char* frames, int nframes, int H, int W, const int* jobs17, int n, int grid,
                       int radius, int* out4, hipStream_t s) {
  GCV_REQUIRE(grid == 16 || grid == 32 || grid == 64, "track match: grid is 16, 32 or 64");
  GCV_REQUIRE(radius >= 0 && radius <= TM_RMAX, "track match: radius is 0 ... 32");
  GCV_REQUIRE(nframes > 0 && H > 0 && W > 0, "track match: bad geometry");
  GCV_REQUIRE((int64_t)H * W <= ((int64_t)1 << 30), "track match: frames of more than 2^30 pixels");   // a cell's sum: 32 bits
  GCV_REQUIRE(n >= 0, "track match: negative job count");
  if (n == 0) return 0;
  if (grid == 16)
    hipLaunchKernelGGL(track_match_kernel<16>, dim3((unsigned)n), dim3(TM_THREADS), 0, s, frames, nframes, H, W, jobs17,
                       radius, out4);
  else if (grid == 32)
    hipLaunchKernelGGL(track_match_kernel<32>, dim3((unsigned)n), dim3(TM_THREADS), 0, s, frames, nframes, H, W, jobs17,
                       radius, out4);
  else
    hipLaunchKernelGGL(track_match_kernel<64>, dim3((unsigned)n), dim3(TM_THREADS), 0, s, frames, nframes, H, W, jobs17,
                       radius, out4);
  GCV_CHECK_HIP(hipGetLastError());
  return 0;
}

}  // namespace gcv
