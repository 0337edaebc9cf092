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
// hist_diff: one wave per (pair, region), lane = bin, |a - b| and a cross-lane sum.
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

__device__ __forceinline__ void fh_tally(uint32_t* s_col, const FhPix& p) {
  constexpr uint32_t WEIGHTS = 77u | 150u << 8 | 29u << 16;               // R, G, B; the fourth byte counts 0
  const uint32_t e0 = __builtin_amdgcn_alignbyte(p.d1, p.d0, p.sh), e1 = __builtin_amdgcn_alignbyte(p.d2, p.d1, p.sh),
                 e2 = __builtin_amdgcn_alignbyte(p.d3, p.d2, p.sh);
  const uint32_t px[4] = {e0, __builtin_amdgcn_alignbyte(e1, e0, 3), __builtin_amdgcn_alignbyte(e2, e1, 2), e2 >> 8};
#pragma unroll
  for (int k = 0; k < 4; ++k)
    if (k < p.np) {
      const uint32_t y256 = __builtin_amdgcn_udot4(px[k], WEIGHTS, 128u, false);     // 77 R + 150 G + 29 B + 128
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

// one wave per (pair p, region r): item = p RR + r, and the same region of the next frame is item + RR
__global__ void __launch_bounds__(FH_THREADS) hist_diff_kernel(const uint32_t* __restrict__ hist, int64_t items, int RR,
                                                               uint32_t* __restrict__ dist) {
  const int64_t item = (int64_t)blockIdx.x * (FH_THREADS / 64) + (threadIdx.x >> 6);
  if (item >= items) return;                               // wave-uniform
  const int lane = threadIdx.x & 63;
  const uint32_t a = hist[item * FH_BINS + lane], b = hist[(item + RR) * FH_BINS + lane];
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

int launch_hist_diff(const uint32_t* hist, int nframes, int regions, uint32_t* dist, hipStream_t s) {
  GCV_REQUIRE(cuts_lg_regions(regions) >= 0, "hist diff: regions is 1, 2, 4 or 8");
  GCV_REQUIRE(nframes > 0, "hist diff: bad geometry");
  const int64_t items = (int64_t)(nframes - 1) * regions * regions;
  GCV_REQUIRE(cdiv64(items, FH_THREADS / 64) <= INT_MAX, "hist diff: too many frames for one launch");
  if (items == 0) return 0;
  hipLaunchKernelGGL(hist_diff_kernel, dim3((unsigned)cdiv64(items, FH_THREADS / 64)), dim3(FH_THREADS), 0, s, hist, items,
                     regions * regions, dist);
  GCV_CHECK_HIP(hipGetLastError());
  return 0;
}

}  // namespace gcv
