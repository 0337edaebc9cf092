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
//
// gcv_track_chain carries a face past its first or last detection with the same three phases (they are __device__
// functions below, one copy for both kernels): one workgroup per chain, the template built once, and a loop over the
// frames of the chain in which each step searches around the box of the step before.  A launch holds a few dozen chains,
// so it is bound by steps x the latency of one step, and a workgroup larger than track_match's 256 threads shortens a
// step (TC_THREADS; the A/B is profiles/extend_threads_ab.json).
#include <cstdint>

#include "common.h"
#include "luma_cells.h"                                   // TmBox, tm_box_ok, tm_cell

namespace gcv {

constexpr int TM_THREADS = 256;
constexpr int TC_THREADS = 1024;                            // profiles/extend_threads_ab.json: 2.78 ms at 256, 1.94 at 512, 1.56
constexpr int TM_RMAX = 32;
constexpr int TC_STEPS_MAX = 1024;

struct alignas(4) TmOut { int v[4]; };
struct TmRange { int dy_lo, dy_hi, dx_lo, dx_hi; };

// ---- the phases, shared by track_match_kernel and track_chain_kernel -------------------------------------------------
// window cell (u, v) sits at byte (u + R) * ws + (v + R) of s_win; ws is a multiple of 4 with 4 spare bytes, G + 68 at most
__device__ __forceinline__ int tm_row_stride(int G, int R) { return ((G + 2 * R + 3) & ~3) + 4; }

// cell edges e(u) = floor(u * extent / G) for u = -R ... G + R at index u + R: the shift is a floor division for negative
// u as well
template <int LG>
__device__ __forceinline__ void tm_edges(int* __restrict__ s_ey, int* __restrict__ s_ex, int h, int w, int G, int R, int tid,
                                         int nt) {
  for (int i = tid; i <= G + 2 * R; i += nt) {
    s_ey[i] = (int)(((int64_t)(i - R) * h) >> LG);
    s_ex[i] = (int)(((int64_t)(i - R) * w) >> LG);
  }
}

// valid displacements: e is monotone, so they are the ranges around 0 in which the displaced box stays in the frame
__device__ __forceinline__ TmRange tm_valid_range(const int* s_ey, const int* s_ex, int top, int bottom, int left, int right,
                                                  int H, int W, int R) {
  TmRange g = {0, 0, 0, 0};
  while (g.dy_lo > -R && top + s_ey[g.dy_lo - 1 + R] >= 0) --g.dy_lo;
  while (g.dy_hi < R && bottom + s_ey[g.dy_hi + 1 + R] <= H) ++g.dy_hi;
  while (g.dx_lo > -R && left + s_ex[g.dx_lo - 1 + R] >= 0) --g.dx_lo;
  while (g.dx_hi < R && right + s_ex[g.dx_hi + 1 + R] <= W) ++g.dx_hi;
  return g;
}

// phase 1, window: cell i of the (dy_hi - dy_lo + G) x (dx_hi - dx_lo + G) cells u in [dy_lo, dy_hi + G), v in
// [dx_lo, dx_hi + G) — together the displaced boxes of the valid candidates, all inside the frame.  One thread = one
// cell; consecutive i are consecutive cells of a cell row.
__device__ __forceinline__ void tm_window_cell(unsigned char* __restrict__ s_win, const int* s_ey, const int* s_ex,
                                               const unsigned char* __restrict__ frame, int64_t rs, int top, int left,
                                               const TmRange& g, int G, int R, int ws, int i) {
  const int nxc = g.dx_hi - g.dx_lo + G;
  const int r = i / nxc, iu = r + g.dy_lo + R, iv = i - r * nxc + g.dx_lo + R;
  s_win[iu * ws + iv] = (unsigned char)tm_cell(frame, rs, top + s_ey[iu], top + s_ey[iu + 1], left + s_ex[iv],
                                               left + s_ex[iv + 1]);
}

// phase 1, template: cell k = u * G + v of a box whose edges (index u = 0 ... G) are ty, tx
template <int G, int LG>
__device__ __forceinline__ void tm_template_cell(unsigned char* __restrict__ s_tpl, const int* ty, const int* tx,
                                                 const unsigned char* __restrict__ frame, int64_t rs, int top, int left,
                                                 int k) {
  const int u = (k >> LG) & (G - 1), v = k & (G - 1);
  s_tpl[u * G + v] = (unsigned char)tm_cell(frame, rs, top + ty[u], top + ty[u + 1], left + tx[v], left + tx[v + 1]);
}

// phase 2: the valid candidates over the lanes, consecutive dx on consecutive lanes; the smallest key of this lane's
// candidates.  TWO = false drops template b and the weights: cost = sum |A - V|.
template <int G, bool TWO>
__device__ __forceinline__ unsigned long long tm_candidates(const unsigned char* __restrict__ s_win,
                                                            const unsigned char* __restrict__ s_ta,
                                                            const unsigned char* __restrict__ s_tb, unsigned wa, unsigned wb,
                                                            const TmRange& g, int R, int ws, unsigned* s_cost0, int tid,
                                                            int nt) {
  unsigned long long best = ~0ull;
  const int nx = g.dx_hi - g.dx_lo + 1, ncand = (g.dy_hi - g.dy_lo + 1) * nx;
  const uint32_t* ta = reinterpret_cast<const uint32_t*>(s_ta);
  const uint32_t* tb = reinterpret_cast<const uint32_t*>(s_tb);
  for (int c = tid; c < ncand; c += nt) {
    const int cy = c / nx, dy = g.dy_lo + cy, dx = g.dx_lo + (c - cy * nx);
    const unsigned sh = (unsigned)(dx + R) & 3u;
    const uint32_t* wrow = reinterpret_cast<const uint32_t*>(s_win + (dy + R) * ws) + ((dx + R) >> 2);
    unsigned sa = 0, sb = 0;
#pragma unroll 1
    for (int u = 0; u < G; ++u, wrow += ws >> 2) {
      uint32_t lo = wrow[0];
#pragma unroll
      for (int q = 0; q < G / 4; ++q) {
        const uint32_t hi = wrow[q + 1];                   // past the last cell for q = G / 4 - 1: inside the row's spare
        const uint32_t v = __builtin_amdgcn_alignbyte(hi, lo, sh);        // bytes, and shifted out again
        sa = __builtin_amdgcn_sad_u8(ta[u * (G / 4) + q], v, sa);
        if (TWO) sb = __builtin_amdgcn_sad_u8(tb[u * (G / 4) + q], v, sb);
        lo = hi;
      }
    }
    const unsigned cost = TWO ? wa * sa + wb * sb : sa;                   // <= 1024 * G * G * 255 < 2^31
    if (dy == 0 && dx == 0) *s_cost0 = cost;
    const unsigned long long key = (unsigned long long)cost << 32 | (unsigned long long)(dy * dy + dx * dx) << 16 |
                                   (unsigned long long)(dy + R) << 8 | (unsigned long long)(dx + R);
    best = key < best ? key : best;
  }
  return best;
}

// phase 3: the smallest key of the workgroup, in every thread: across each wave by shuffles, across the waves through LDS.
// The barrier inside also orders phase 2's LDS reads (and its write of cost0) before whatever the caller does next.
template <int NT>
__device__ __forceinline__ unsigned long long tm_min_key(unsigned long long best, unsigned long long* s_key, int tid) {
#pragma unroll
  for (int m = 32; m >= 1; m >>= 1) {
    const unsigned long long o = __shfl_xor(best, m, 64);
    best = o < best ? o : best;
  }
  if ((tid & 63) == 0) s_key[tid >> 6] = best;
  __syncthreads();
  best = s_key[0];
#pragma unroll
  for (int k = 1; k < NT / 64; ++k) best = s_key[k] < best ? s_key[k] : best;
  return best;
}

template <int G>
__global__ void __launch_bounds__(TM_THREADS) track_match_kernel(const unsigned char* __restrict__ frames, int nframes,
                                                                 int H, int W, const int* __restrict__ jobs, int R,
                                                                 int* __restrict__ out) {
  constexpr int LG = G == 16 ? 4 : (G == 32 ? 5 : 6);
  constexpr int NE = G + 2 * TM_RMAX + 1;                  // edges of the window cells u = -R ... G + R
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

  tm_edges<LG>(s_ey, s_ex, h, w, G, R, tid, TM_THREADS);
  for (int i = tid; i < 2 * (G + 1); i += TM_THREADS) {
    const int t = i > G, u = t ? i - (G + 1) : i;
    s_ty[t][u] = (int)(((int64_t)u * (t ? b.bottom - b.top : a.bottom - a.top)) >> LG);
    s_tx[t][u] = (int)(((int64_t)u * (t ? b.right - b.left : a.right - a.left)) >> LG);
  }
  __syncthreads();

  const TmRange g = tm_valid_range(s_ey, s_ex, p.top, p.bottom, p.left, p.right, H, W, R);
  const int ws = tm_row_stride(G, R);

  // phase 1: the window cells and the two templates, dealt over the threads as one list
  {
    const int64_t rs = (int64_t)W * 3;
    const int nwin = (g.dy_hi - g.dy_lo + G) * (g.dx_hi - g.dx_lo + G);
    for (int i = tid; i < nwin + 2 * G * G; i += TM_THREADS) {
      if (i < nwin) {
        tm_window_cell(s_win, s_ey, s_ex, frames + (int64_t)p.f * H * rs, rs, p.top, p.left, g, G, R, ws, i);
      } else {
        const int k = i - nwin, t = k >> (2 * LG);
        tm_template_cell<G, LG>(s_tpl[t], s_ty[t], s_tx[t], frames + (int64_t)(t ? b.f : a.f) * H * rs, rs,
                                t ? b.top : a.top, t ? b.left : a.left, k);
      }
    }
  }
  __syncthreads();

  // phase 2 and 3
  unsigned long long best = tm_candidates<G, true>(s_win, s_tpl[0], s_tpl[1], (unsigned)wa, (unsigned)wb, g, R, ws, &s_cost0,
                                                   tid, TM_THREADS);
  best = tm_min_key<TM_THREADS>(best, s_key, tid);
  if (tid == 0) {
    const int dy = (int)(best >> 8 & 0xFFu), dx = (int)(best & 0xFFu);   // still offset by R: the index of the edge
    *dst = TmOut{{s_ey[dy], s_ex[dx], (int)(best >> 32), (int)s_cost0}};
  }
}

// gcv_track_chain: one workgroup walks one chain.  The template's cells are built once and stay in LDS; every step
// rebuilds the window cells of its frame around the box the step before found, runs the candidates, and takes the
// workgroup's smallest key in every thread (tm_min_key), so all waves agree on the next prior and on the exit at stop.
// The template and the window have the same h and w: the template's edges are the window's, s_ey + R and s_ex + R.
// Across steps: a step's candidate reads of s_win end before tm_min_key's barrier, the next step's window writes come
// after it; s_key and s_cost0 are read behind that barrier and next written behind the next step's phase-1 barrier.
template <int G, int NT>
__global__ void __launch_bounds__(NT) track_chain_kernel(const unsigned char* __restrict__ frames, int nframes, int H, int W,
                                                         const int* __restrict__ jobs, int R, int max_steps,
                                                         int* __restrict__ out) {
  constexpr int LG = G == 16 ? 4 : (G == 32 ? 5 : 6);
  constexpr int NE = G + 2 * TM_RMAX + 1;
  __shared__ __attribute__((aligned(16))) unsigned char s_win[(G + 2 * TM_RMAX) * (G + 2 * TM_RMAX + 4)];
  __shared__ __attribute__((aligned(16))) unsigned char s_tpl[G * G];
  __shared__ int s_ey[NE], s_ex[NE];
  __shared__ unsigned long long s_key[NT / 64];
  __shared__ unsigned s_cost0;

  const int tid = threadIdx.x;
  const int* j = jobs + 11 * (size_t)blockIdx.x;
  const TmBox a = {j[0], j[1], j[2], j[3], j[4]};
  const int fs = j[5], dir = j[6], steps = j[7], py = j[8], px = j[9], stop = j[10];
  TmOut* dst = reinterpret_cast<TmOut*>(out) + (size_t)max_steps * blockIdx.x;
  const TmOut none = {{0, 0, -1, -1}};
  // a bad row (block-uniform): read nothing, write the refusal row throughout.  steps <= 1024 and 0 <= fs < nframes keep
  // fs + dir (steps - 1) inside an int
  const bool ok = tm_box_ok(a, nframes, H, W, G) && (dir == 1 || dir == -1) && steps >= 1 && steps <= max_steps && stop >= 0 &&
                  fs >= 0 && fs < nframes && fs + dir * (steps - 1) >= 0 && fs + dir * (steps - 1) < nframes &&
                  (int64_t)a.top + py >= 0 && (int64_t)a.bottom + py <= H && (int64_t)a.left + px >= 0 &&
                  (int64_t)a.right + px <= W;
  if (!ok) {
    for (int k = tid; k < max_steps; k += NT) dst[k] = none;
    return;
  }
  const int h = a.bottom - a.top, w = a.right - a.left, ws = tm_row_stride(G, R);
  const int64_t rs = (int64_t)W * 3;

  tm_edges<LG>(s_ey, s_ex, h, w, G, R, tid, NT);
  __syncthreads();
  for (int k = tid; k < G * G; k += NT)
    tm_template_cell<G, LG>(s_tpl, s_ey + R, s_ex + R, frames + (int64_t)a.f * H * rs, rs, a.top, a.left, k);

  int top = a.top + py, left = a.left + px, k = 0;
  for (; k < steps; ++k) {
    const TmRange g = tm_valid_range(s_ey, s_ex, top, top + h, left, left + w, H, W, R);
    const unsigned char* frame = frames + (int64_t)(fs + dir * k) * H * rs;
    const int nwin = (g.dy_hi - g.dy_lo + G) * (g.dx_hi - g.dx_lo + G);
    for (int i = tid; i < nwin; i += NT) tm_window_cell(s_win, s_ey, s_ex, frame, rs, top, left, g, G, R, ws, i);
    __syncthreads();
    unsigned long long best = tm_candidates<G, false>(s_win, s_tpl, s_tpl, 1u, 0u, g, R, ws, &s_cost0, tid, NT);
    best = tm_min_key<NT>(best, s_key, tid);
    if ((int)(best >> 32) > stop) break;                   // the same key in every thread: the whole workgroup leaves
    const int oy = s_ey[(int)(best >> 8 & 0xFFu)], ox = s_ex[(int)(best & 0xFFu)];
    if (tid == 0) dst[k] = TmOut{{oy, ox, (int)(best >> 32), (int)s_cost0}};
    top += oy;
    left += ox;
  }
  for (int i = k + tid; i < max_steps; i += NT) dst[i] = none;
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

int launch_track_chain(const unsigned char* frames, int nframes, int H, int W, const int* jobs11, int n, int max_steps,
                       int grid, int radius, int* out4, hipStream_t s) {
  GCV_REQUIRE(grid == 16 || grid == 32 || grid == 64, "track chain: grid is 16, 32 or 64");
  GCV_REQUIRE(radius >= 0 && radius <= TM_RMAX, "track chain: radius is 0 ... 32");
  GCV_REQUIRE(max_steps >= 1 && max_steps <= TC_STEPS_MAX, "track chain: max_steps is 1 ... 1024");
  GCV_REQUIRE(nframes > 0 && H > 0 && W > 0, "track chain: bad geometry");
  GCV_REQUIRE((int64_t)H * W <= ((int64_t)1 << 30), "track chain: frames of more than 2^30 pixels");
  GCV_REQUIRE(n >= 0, "track chain: negative job count");
  if (n == 0) return 0;
  if (grid == 16)
    hipLaunchKernelGGL((track_chain_kernel<16, TC_THREADS>), dim3((unsigned)n), dim3(TC_THREADS), 0, s, frames, nframes, H, W,
                       jobs11, radius, max_steps, out4);
  else if (grid == 32)
    hipLaunchKernelGGL((track_chain_kernel<32, TC_THREADS>), dim3((unsigned)n), dim3(TC_THREADS), 0, s, frames, nframes, H, W,
                       jobs11, radius, max_steps, out4);
  else
    hipLaunchKernelGGL((track_chain_kernel<64, TC_THREADS>), dim3((unsigned)n), dim3(TC_THREADS), 0, s, frames, nframes, H, W,
                       jobs11, radius, max_steps, out4);
  GCV_CHECK_HIP(hipGetLastError());
  return 0;
}

}  // namespace gcv
