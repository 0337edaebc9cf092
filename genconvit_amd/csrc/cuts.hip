// Shot cuts: per-region luma histograms of every frame and their L1 distance between consecutive frames (gcv_frame_hist,
// gcv_hist_diff, include/genconvit_hip.h, which fixes the arithmetic; tests/cutsutil.py restates it bit for bit).  A
// whole-video scan links faces into tracks by position alone; across a hard cut the face of another person often sits
// where the last one sat.  The histograms say where the shots end, and pred_func.shot_cuts turns the distances into cuts.
//
// frame_hist is the streaming one: every pixel of every frame is read once.
//   * A workgroup of 256 threads takes a run of pixel rows of one region of one frame: the whole region (plain stores of
//     its 64 counts, no memset, no global atomics), or, when frames x regions alone would leave most of the 256 CUs idle
//     (few frames, R = 1 or 2), one of S row slices of it, merged by integer atomicAdd into a zeroed output — integer adds
//     commute, so the result does not depend on the order.
//   * A pixel row of a region is a run of 3 w bytes that starts at any byte, and the frames' base pointer need not be
//     dword-aligned.  A lane takes 4 pixels = 12 bytes: it reads the 4 aligned dwords around them in one load (consecutive
//     lanes 12 bytes apart: a wave's load is one contiguous run of 772 bytes) and shifts the 12 bytes out with three
//     v_alignbyte_b32; the shift is the same for a whole row.  The aligned dwords of a lane may start before the first
//     byte of the frames or end behind the last one (only the first and the last 16 bytes of the buffer can do that):
//     such a lane reads its pixels byte by byte instead, so nothing outside the buffer is ever read.
//   * Luma: one v_alignbyte_b32 puts a pixel's R, G, B into the low three bytes of a dword, one v_dot4_u32_u8 with the
//     weights (77, 150, 29, 0) and the accumulator 128 gives 256 Y + rest; bin = that >> 10.
//   * The histogram lives in LDS as s_h[bin][32], updated by ds_add_u32; a lane adds to column lane & 31.  The 32 lanes
//     that the LDS serves in one cycle therefore sit on 32 different banks whatever the picture shows — neighbouring
//     pixels of a natural image fall into the same bin, which on a single 64-bin histogram is one address for the whole
//     wave.  The four waves share the 8 KB table (the adds are atomic), so eight workgroups fit a CU.
//   * At the end four lanes sum the 32 columns of a bin, two shuffles, one store (or atomicAdd) per bin.
// hist_diff: one wave per (pair, region), lane = bin, |a - b| and a cross-lane sum; hist_diff_lag is the same kernel with
// the second frame lag frames on.
//
// Fades and dissolves (gcv_frame_cells, gcv_blend_fit, gcv_hist_diff_lag; tests/transutil.py restates them): the frames of
// a linear blend lie, as vectors of luma sums over a G x G grid of cells, on the straight line between the two ends.
// frame_cells is frame_hist's streaming pass with sums in place of counts:
//   * A workgroup takes a run of pixel rows of one row of cells of one frame, the whole width of the picture (or one of S
//     slices of it, merged by atomicAdd into a zeroed output, where frames x G leaves the chip idle), with the same loads.
//   * A lane adds the lumas of its 4 pixels and gives the sum to the cell of the first pixel with one ds_add_u32 on
//     s_c[cell][32], column lane & 31 as above; that cell comes from one division, v = ((x + 1) G - 1) / W, the next edges
//     from a table in LDS.  A group that crosses an edge hands over what it has and goes on in the next cell, at every edge
//     it crosses: at G = 32 on small frames a group holds two whole cells.
// blend_fit: one workgroup per span; A and D = B - A stay in registers (1 or 4 cells a thread), every row between the
// ends is loaded once, coalesced, the int64 products are summed across the wave by shuffles and across the waves in LDS.
// No scratch, nothing allocated or synchronised; the only other call on the stream is the memset of a split launch.
#include <algorithm>
#include <climits>
#include <cstdint>

#include "common.h"

namespace gcv {

constexpr int FH_THREADS = 256;
constexpr int FH_BINS = 64;
constexpr int FH_COLS = 32;                                // columns of a bin in LDS: one per bank
constexpr int FH_TARGET_WGS = 1024;                        // split regions until about 4 workgroups a CU exist ...
constexpr int FH_MIN_ROWS = 8;                             // ... but leave every slice at least 8 pixel rows

constexpr int FC_MAX_GRID = 32;                           // frame_cells: G = 8, 16 or 32 cells a side
constexpr int BF_THREADS = 256;
constexpr int BF_MAX_LAG = 32;                             // blend_fit: a span has 2 lag - 1 <= 63 sums

struct alignas(4) FhQuad { uint32_t d[4]; };

// 4 pixels as loaded: the 12 bytes R0 G0 B0 R1 ... B3 start sh bytes into the 16 bytes d0 ... d3; np of the pixels count
struct FhPix { uint32_t d0, d1, d2, d3; unsigned sh; int np; };

// the 4 pixels from byte offset o of the frames (np of them inside the row); sh = (address of that byte) & 3.  Only the
// load is here and the shifts are in fh_tally, so that a lane's second load is issued before it waits for the first.
__device__ __forceinline__ FhPix fh_load(const unsigned char* __restrict__ frames, int64_t nbytes, int64_t o, unsigned sh,
                                         int np) {
  FhPix r = {0u, 0u, 0u, 0u, sh, np};
  const int64_t oa = o - (int64_t)sh;                      // the aligned dword that holds the first byte
  if (oa >= 0 && oa + 16 <= nbytes) {
    const FhQuad q = *reinterpret_cast<const FhQuad*>(frames + oa);
    r.d0 = q.d[0], r.d1 = q.d[1], r.d2 = q.d[2], r.d3 = q.d[3];
  } else {                                                 // the first or last 16 bytes of the buffer: only the pixels' bytes
    const int nb = 3 * np;
    r.sh = 0u;
#pragma unroll
    for (int b = 0; b < 12; ++b) {
      const uint32_t v = b < nb ? (uint32_t)frames[o + b] << (8 * (b & 3)) : 0u;
      if (b < 4) r.d0 |= v;
      else if (b < 8) r.d1 |= v;
      else r.d2 |= v;
    }
  }
  return r;
}

// the 4 pixels of a loaded group, each as R, G, B in the low three bytes of a dword
__device__ __forceinline__ void fh_unpack(const FhPix& p, uint32_t (&px)[4]) {
  const uint32_t e0 = __builtin_amdgcn_alignbyte(p.d1, p.d0, p.sh), e1 = __builtin_amdgcn_alignbyte(p.d2, p.d1, p.sh),
                 e2 = __builtin_amdgcn_alignbyte(p.d3, p.d2, p.sh);
  px[0] = e0, px[1] = __builtin_amdgcn_alignbyte(e1, e0, 3), px[2] = __builtin_amdgcn_alignbyte(e2, e1, 2), px[3] = e2 >> 8;
}

constexpr uint32_t FH_WEIGHTS = 77u | 150u << 8 | 29u << 16;              // R, G, B; the fourth byte counts 0

__device__ __forceinline__ void fh_tally(uint32_t* s_col, const FhPix& p) {
  uint32_t px[4];
  fh_unpack(p, px);
#pragma unroll
  for (int k = 0; k < 4; ++k)
    if (k < p.np) {
      const uint32_t y256 = __builtin_amdgcn_udot4(px[k], FH_WEIGHTS, 128u, false);  // 77 R + 150 G + 29 B + 128
      atomicAdd(s_col + (y256 >> 10) * FH_COLS, 1u);                                  // bin = Y >> 2 = y256 >> 10
    }
}

// blockIdx.x = ((f R + u) R + v) S + s: slice s of region (u, v) of frame f
__global__ void __launch_bounds__(FH_THREADS) frame_hist_kernel(const unsigned char* __restrict__ frames, int64_t nbytes,
                                                                int H, int W, int lgR, int S, uint32_t* __restrict__ hist) {
  __shared__ uint32_t s_h[FH_BINS * FH_COLS];
  const int tid = threadIdx.x;
  const unsigned R = 1u << lgR;
  const unsigned fr = blockIdx.x / (unsigned)S, s = blockIdx.x - fr * (unsigned)S;
  const unsigned v = fr & (R - 1u), u = (fr >> lgR) & (R - 1u), f = fr >> (2 * lgR);
  const int ry0 = (int)(((int64_t)u * H) >> lgR), ry1 = (int)(((int64_t)(u + 1u) * H) >> lgR);
  const int x0 = (int)(((int64_t)v * W) >> lgR), x1 = (int)(((int64_t)(v + 1u) * W) >> lgR);
  const int ya = ry0 + (int)((int64_t)s * (ry1 - ry0) / S), yb = ry0 + (int)((int64_t)(s + 1u) * (ry1 - ry0) / S);
  const int w = x1 - x0, n = yb - ya, g = (w + 3) >> 2;   // n rows of g groups of 4 pixels

  for (int i = tid; i < FH_BINS * FH_COLS; i += FH_THREADS) s_h[i] = 0u;
  __syncthreads();

  // the groups of the slice are dealt over the threads row-major; a thread walks (row, i) in steps of 256 groups
  const int dq = FH_THREADS / g, dr = FH_THREADS % g;
  int row = tid / g, i = tid % g;
  const int64_t rs = (int64_t)W * 3;
  const int64_t o00 = ((int64_t)f * H + ya) * rs + (int64_t)x0 * 3;       // first byte of the slice
  const unsigned mis = (unsigned)(reinterpret_cast<uintptr_t>(frames) & 3u);
  uint32_t* s_col = s_h + (tid & (FH_COLS - 1));
  auto next = [&](FhPix& p) {                              // load this thread's next group (np = 0 behind the end), step on
    p = FhPix{0u, 0u, 0u, 0u, 0u, 0};
    if (row < n) {
      const int64_t o = o00 + (int64_t)row * rs + 12 * (int64_t)i;
      p = fh_load(frames, nbytes, o, (mis + (unsigned)o) & 3u, min(4, w - 4 * i));
    }
    row += dq;
    i += dr;
    if (i >= g) { i -= g; ++row; }
  };
  while (row < n) {                                        // two loads in flight per lane
    FhPix a, b;
    next(a);
    next(b);
    fh_tally(s_col, a);
    fh_tally(s_col, b);
  }
  __syncthreads();

  // bin = tid / 4; four lanes sum eight columns each
  uint32_t c = 0;
#pragma unroll
  for (int k = 0; k < FH_COLS / 4; ++k) c += s_h[(tid >> 2) * FH_COLS + (tid & 3) * (FH_COLS / 4) + k];
  c += __shfl_xor(c, 1, 64);
  c += __shfl_xor(c, 2, 64);
  if ((tid & 3) == 0) {
    uint32_t* dst = hist + (size_t)fr * FH_BINS + (tid >> 2);
    if (S == 1) *dst = c;
    else if (c) atomicAdd(dst, c);
  }
}

// blockIdx.x = (f G + u) S + s: slice s of the cell row u (G cells side by side, the whole width of the picture) of frame f
__global__ void __launch_bounds__(FH_THREADS) frame_cells_kernel(const unsigned char* __restrict__ frames, int64_t nbytes,
                                                                 int H, int W, int lgG, int S, uint32_t* __restrict__ cells) {
  __shared__ uint32_t s_c[FC_MAX_GRID * FH_COLS];
  __shared__ int s_ex[FC_MAX_GRID + 1];                    // the column edges (v W) // G
  const int tid = threadIdx.x;
  const unsigned G = 1u << lgG;
  const unsigned fu = blockIdx.x / (unsigned)S, s = blockIdx.x - fu * (unsigned)S;
  const unsigned u = fu & (G - 1u), f = fu >> lgG;
  const int ry0 = (int)(((int64_t)u * H) >> lgG), ry1 = (int)(((int64_t)(u + 1u) * H) >> lgG);
  const int ya = ry0 + (int)((int64_t)s * (ry1 - ry0) / S), yb = ry0 + (int)((int64_t)(s + 1u) * (ry1 - ry0) / S);
  const int n = yb - ya, g = (W + 3) >> 2;                 // n rows of g groups of 4 pixels

  for (int i = tid; i < (int)G * FH_COLS; i += FH_THREADS) s_c[i] = 0u;
  if (tid <= (int)G) s_ex[tid] = (int)(((int64_t)tid * W) >> lgG);
  __syncthreads();

  // the groups of the slice are dealt over the threads row-major, as in frame_hist_kernel
  const int dq = FH_THREADS / g, dr = FH_THREADS % g;
  int row = tid / g, i = tid % g;
  const int64_t rs = (int64_t)W * 3;
  const int64_t o00 = ((int64_t)f * H + ya) * rs;          // first byte of the slice
  const unsigned mis = (unsigned)(reinterpret_cast<uintptr_t>(frames) & 3u);
  uint32_t* s_col = s_c + (tid & (FH_COLS - 1));
  auto next = [&](FhPix& p, int& x) {                      // load this thread's next group (np = 0 behind the end), step on
    p = FhPix{0u, 0u, 0u, 0u, 0u, 0};
    x = 4 * i;
    if (row < n) {
      const int64_t o = o00 + (int64_t)row * rs + 12 * (int64_t)i;
      p = fh_load(frames, nbytes, o, (mis + (unsigned)o) & 3u, min(4, W - 4 * i));
    }
    row += dq;
    i += dr;
    if (i >= g) { i -= g; ++row; }
  };
  // a group adds its lumas to the cell of its first pixel, x in [s_ex[v], s_ex[v + 1]) <=> v = ((x + 1) G - 1) // W, and moves
  // on to the next cell at every edge it crosses (W >= G: a cell is at least one pixel wide, so one step per pixel does)
  auto tally = [&](const FhPix& p, int x) {
    if (p.np == 0) return;
    uint32_t px[4];
    fh_unpack(p, px);
    int v = (int)(((((unsigned)x + 1u) << lgG) - 1u) / (unsigned)W);
    int edge = s_ex[v + 1];
    uint32_t acc = 0u;
#pragma unroll
    for (int k = 0; k < 4; ++k)
      if (k < p.np) {
        if (x + k >= edge) {
          atomicAdd(s_col + v * FH_COLS, acc);
          acc = 0u;
          edge = s_ex[++v + 1];
        }
        acc += __builtin_amdgcn_udot4(px[k], FH_WEIGHTS, 128u, false) >> 8;          // Y
      }
    atomicAdd(s_col + v * FH_COLS, acc);
  };
  while (row < n) {                                        // two loads in flight per lane
    FhPix a, b;
    int xa, xb;
    next(a, xa);
    next(b, xb);
    tally(a, xa);
    tally(b, xb);
  }
  __syncthreads();

  // cell = tid / 4; four lanes sum eight columns each
  uint32_t c = 0;
  if (tid < 4 * (int)G) {
#pragma unroll
    for (int k = 0; k < FH_COLS / 4; ++k) c += s_c[(tid >> 2) * FH_COLS + (tid & 3) * (FH_COLS / 4) + k];
  }
  c += __shfl_xor(c, 1, 64);
  c += __shfl_xor(c, 2, 64);
  if (tid < 4 * (int)G && (tid & 3) == 0) {
    uint32_t* dst = cells + ((size_t)fu << lgG) + (tid >> 2);
    if (S == 1) *dst = c;
    else if (c) atomicAdd(dst, c);
  }
}

__device__ __forceinline__ int64_t bf_wave_sum(int64_t v) {
#pragma unroll
  for (int m = 32; m >= 1; m >>= 1) v += __shfl_xor(v, m, 64);
  return v;
}

// one workgroup per span p = blockIdx.x: blockDim.x = min(256, G G) threads hold NPT = G G / blockDim.x cells each of
// A = cells[p] and D = cells[p + lag] - A in registers, and walk the rows between the two
template <int NPT>
__global__ void __launch_bounds__(BF_THREADS) blend_fit_kernel(const uint32_t* __restrict__ cells, int GG, int lag,
                                                               int64_t* __restrict__ fit) {
  __shared__ int64_t s_part[BF_THREADS / 64][2 * BF_MAX_LAG - 1];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, nt = blockDim.x;
  const uint32_t* __restrict__ rowA = cells + (int64_t)blockIdx.x * GG;
  int64_t a[NPT], d[NPT], dd = 0;
#pragma unroll
  for (int j = 0; j < NPT; ++j) {
    a[j] = (int64_t)rowA[tid + j * nt];
    d[j] = (int64_t)rowA[(int64_t)lag * GG + tid + j * nt] - a[j];
    dd += d[j] * d[j];
  }
  dd = bf_wave_sum(dd);
  if (lane == 0) s_part[wave][0] = dd;
  for (int k = 1; k < lag; ++k) {
    int64_t md = 0, mm = 0;
#pragma unroll
    for (int j = 0; j < NPT; ++j) {
      const int64_t m = (int64_t)rowA[(int64_t)k * GG + tid + j * nt] - a[j];
      md += m * d[j];
      mm += m * m;
    }
    md = bf_wave_sum(md);
    mm = bf_wave_sum(mm);
    if (lane == 0) s_part[wave][k] = md, s_part[wave][lag - 1 + k] = mm;
  }
  __syncthreads();
  if (tid < 2 * lag - 1) {                                 // at most 63: inside the first wave
    int64_t v = 0;
    for (int w = 0; w < (nt >> 6); ++w) v += s_part[w][tid];
    fit[(int64_t)blockIdx.x * (2 * lag - 1) + tid] = v;
  }
}

// one wave per (pair p, region r): item = p RR + r, and the same region of frame p + lag is item + step, step = lag RR
__global__ void __launch_bounds__(FH_THREADS) hist_diff_kernel(const uint32_t* __restrict__ hist, int64_t items, int64_t step,
                                                               uint32_t* __restrict__ dist) {
  const int64_t item = (int64_t)blockIdx.x * (FH_THREADS / 64) + (threadIdx.x >> 6);
  if (item >= items) return;                               // wave-uniform
  const int lane = threadIdx.x & 63;
  const uint32_t a = hist[item * FH_BINS + lane], b = hist[(item + step) * FH_BINS + lane];
  uint32_t d = a > b ? a - b : b - a;
#pragma unroll
  for (int m = 32; m >= 1; m >>= 1) d += __shfl_xor(d, m, 64);
  if (lane == 0) dist[item] = d;
}

static int cuts_lg_regions(int regions) { return regions == 1 ? 0 : regions == 2 ? 1 : regions == 4 ? 2 : regions == 8 ? 3 : -1; }

int launch_frame_hist(const unsigned char* frames, int nframes, int H, int W, int regions, uint32_t* hist, hipStream_t s) {
  const int lgR = cuts_lg_regions(regions);
  GCV_REQUIRE(lgR >= 0, "frame hist: regions is 1, 2, 4 or 8");
  GCV_REQUIRE(nframes > 0 && H > 0 && W > 0, "frame hist: bad geometry");
  GCV_REQUIRE(H >= regions && W >= regions, "frame hist: a frame smaller than its grid of regions");
  GCV_REQUIRE((int64_t)H * W <= ((int64_t)1 << 30), "frame hist: frames of more than 2^30 pixels");   // a count: 32 bits
  const int64_t regs = (int64_t)nframes * regions * regions;
  int S = 1;                                               // every region has at least H / regions rows
  if (regs < FH_TARGET_WGS) S = (int)std::min<int64_t>(cdiv64(FH_TARGET_WGS, regs), std::max(1, H / regions / FH_MIN_ROWS));
  GCV_REQUIRE(regs * S <= INT_MAX, "frame hist: too many frames for one launch");
  if (S > 1) GCV_CHECK_HIP(hipMemsetAsync(hist, 0, (size_t)regs * FH_BINS * sizeof(uint32_t), s));
  hipLaunchKernelGGL(frame_hist_kernel, dim3((unsigned)(regs * S)), dim3(FH_THREADS), 0, s, frames,
                     (int64_t)nframes * H * W * 3, H, W, lgR, S, hist);
  GCV_CHECK_HIP(hipGetLastError());
  return 0;
}

int launch_hist_diff_lag(const uint32_t* hist, int nframes, int regions, int lag, uint32_t* dist, hipStream_t s) {
  GCV_REQUIRE(cuts_lg_regions(regions) >= 0, "hist diff: regions is 1, 2, 4 or 8");
  GCV_REQUIRE(nframes > 0 && lag > 0, "hist diff: bad geometry");
  const int64_t items = (int64_t)std::max(0, nframes - lag) * regions * regions;
  GCV_REQUIRE(cdiv64(items, FH_THREADS / 64) <= INT_MAX, "hist diff: too many frames for one launch");
  if (items == 0) return 0;
  hipLaunchKernelGGL(hist_diff_kernel, dim3((unsigned)cdiv64(items, FH_THREADS / 64)), dim3(FH_THREADS), 0, s, hist, items,
                     (int64_t)lag * regions * regions, dist);
  GCV_CHECK_HIP(hipGetLastError());
  return 0;
}

int launch_hist_diff(const uint32_t* hist, int nframes, int regions, uint32_t* dist, hipStream_t s) {
  return launch_hist_diff_lag(hist, nframes, regions, 1, dist, s);
}

int launch_frame_cells(const unsigned char* frames, int nframes, int H, int W, int grid, uint32_t* cells, hipStream_t s) {
  const int lgG = grid == 8 ? 3 : grid == 16 ? 4 : grid == 32 ? 5 : -1;
  GCV_REQUIRE(lgG >= 0, "frame cells: grid is 8, 16 or 32");
  GCV_REQUIRE(nframes > 0 && H > 0 && W > 0, "frame cells: bad geometry");
  GCV_REQUIRE(H >= grid && W >= grid, "frame cells: a frame smaller than its grid of cells");
  // a cell holds fewer than 4 H W / G^2 <= H W / 16 pixels, so a row of cells has a sum of squares below
  // 255^2 (H W)^2 / 16 < 2^62: what blend_fit's 64-bit sums need (include/genconvit_hip.h)
  GCV_REQUIRE((int64_t)H * W <= ((int64_t)1 << 25), "frame cells: frames of more than 2^25 pixels");
  const int64_t rows = (int64_t)nframes * grid;
  int S = 1;                                               // every cell row has at least H / grid pixel rows
  if (rows < FH_TARGET_WGS) S = (int)std::min<int64_t>(cdiv64(FH_TARGET_WGS, rows), std::max(1, H / grid / FH_MIN_ROWS));
  GCV_REQUIRE(rows * S <= INT_MAX, "frame cells: too many frames for one launch");
  if (S > 1) GCV_CHECK_HIP(hipMemsetAsync(cells, 0, (size_t)rows * grid * sizeof(uint32_t), s));
  hipLaunchKernelGGL(frame_cells_kernel, dim3((unsigned)(rows * S)), dim3(FH_THREADS), 0, s, frames,
                     (int64_t)nframes * H * W * 3, H, W, lgG, S, cells);
  GCV_CHECK_HIP(hipGetLastError());
  return 0;
}

int launch_blend_fit(const uint32_t* cells, int nframes, int grid, int lag, int64_t* fit, hipStream_t s) {
  GCV_REQUIRE(grid == 8 || grid == 16 || grid == 32, "blend fit: grid is 8, 16 or 32");
  GCV_REQUIRE(lag >= 2 && lag <= BF_MAX_LAG, "blend fit: lag lies in 2 ... 32");
  GCV_REQUIRE(nframes > 0, "blend fit: bad geometry");
  if (nframes <= lag) return 0;
  const int GG = grid * grid, spans = nframes - lag;
  if (GG <= BF_THREADS)
    hipLaunchKernelGGL(blend_fit_kernel<1>, dim3((unsigned)spans), dim3(GG), 0, s, cells, GG, lag, fit);
  else
    hipLaunchKernelGGL(blend_fit_kernel<FC_MAX_GRID * FC_MAX_GRID / BF_THREADS>, dim3((unsigned)spans), dim3(BF_THREADS), 0, s,
                       cells, GG, lag, fit);
  GCV_CHECK_HIP(hipGetLastError());
  return 0;
}

}  // namespace gcv
