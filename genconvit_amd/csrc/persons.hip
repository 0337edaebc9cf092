// Who is it: an appearance signature of n face boxes (gcv_face_signature) and, for every pair of tracks, the distance of
// their two most alike crops (gcv_sig_link).  include/genconvit_hip.h fixes the arithmetic of both; tests/personutil.py
// restates it bit for bit.  A whole-video scan ends a track at every cut, so an interview that cuts between two speakers
// comes back as dozens of short tracks; pred_func.link_tracks joins them into persons by the distances this returns.
//
// face_signature_kernel: one workgroup of 256 threads per box.
//   1. one thread = one cell of the 16 x 16 grid; consecutive lanes take consecutive cells of a cell row, so a wave's reads
//      of one pixel row are one contiguous run of RGB bytes (quality.hip, phase 1).  The SAME pass over the pixels gives the
//      thread its cell's sums of Cb and Cr: e8(i) = (i h) >> 3 = (2 i h) >> 4 = e16(2 i), so a cell of the 8-grid is exactly
//      four cells of the 16-grid, and every pixel is read once.
//   2. S1 = sum of c and A = sum of |256 c - S1|: across the wave by shuffles, across the four waves through LDS; every
//      thread then normalises and stores its own byte.
//   3. threads 0 ... 127: one chroma cell each (Cb 0 ... 63, Cr 64 ... 127), the four 16-grid sums added from LDS.
// No atomics, no scratch, nothing allocated or synchronised.
//
// sig_link_kernel: one workgroup of 256 threads per pair of 64-row tiles (I, J), I <= J (the grid is square; a workgroup
// with J < I returns at once).  Both tiles' signatures sit in LDS as rows of 96 dwords at a stride of SL_STRIDE = 100
// dwords (2 x 25 600 bytes).  Thread (ti, tj) = (tid / 16, tid % 16) takes the 4 x 4 pairs of the rows i = 4 ti + x of
// tile I and j = tj + 16 y of tile J and reads 16 bytes of each of its eight rows per step (ds_read_b128), 64 v_sad_u8
// per 8 reads, 24 steps.
//   LDS banks (MI355X: a ds_read_b128 of a wave is served in four groups of 16 lanes — {0-3, 12-15, 20-27}, {4-11, 16-19,
//   28-31} and the same + 32 — over 64 dword banks, bank = dword address mod 64; equal addresses broadcast):
//     rows of tile J: every group holds each tj = 0 ... 15 once.  Lane tj reads the dwords 100 (tj + 16 y) + 4 q ... + 3,
//       and 100 tj mod 64 = 4 (9 tj mod 16) runs through all 16 multiples of 4 (9 is odd): 16 lanes x 4 dwords cover the
//       64 banks once each.  At the unpadded stride 96 = 32 mod 64 the 16 rows would fall on two bank quads, 8-way.
//     rows of tile I: a group holds two values of ti (lanes 0-15 and 16-31 of a half wave), i.e. two distinct addresses
//       400 dwords apart = 16 mod 64: different banks; the lanes of one ti broadcast.
//   Any stride of 4 x odd dwords does this; 100 is the smallest above 96 and keeps rows 16-byte aligned.
// Results reach out[a][b] and out[b][a] by atomicMin on global uint32 (a vector atomic; a minimum does not depend on the
// order, so the result is deterministic), reduced first: a thread whose four i rows have one owner takes the minimum down
// its column, and a wave merges equal (owner i, owner j) keys over a shuffle butterfly — when the key is the same in the
// whole wave (rows sorted by track, the usual case) one lane issues the two atomics, otherwise every lane with a valid
// key does.  Rows past n, rows with an owner outside [0, T) and pairs of equal owner contribute nothing.  No scratch.
#include <cstdint>

#include "common.h"
#include "luma_cells.h"                                   // TmBox, tm_box_ok, tm_cell_ycc

namespace gcv {

constexpr int FS_THREADS = 256;
constexpr int FS_BYTES = 384;                             // 16 x 16 luma, 8 x 8 Cb, 8 x 8 Cr

// the sum of v over the workgroup, in every thread; part: 4 words of LDS that nobody else touches until the next barrier
__device__ __forceinline__ unsigned fs_block_sum(unsigned v, unsigned* part, int tid) {
#pragma unroll
  for (int m = 32; m >= 1; m >>= 1) v += __shfl_xor(v, m, 64);
  if ((tid & 63) == 0) part[tid >> 6] = v;
  __syncthreads();
  return part[0] + part[1] + part[2] + part[3];
}

__global__ void __launch_bounds__(FS_THREADS) face_signature_kernel(const unsigned char* __restrict__ frames, int nframes,
                                                                    int H, int W, const int* __restrict__ boxes,
                                                                    unsigned char* __restrict__ out) {
  __shared__ int s_ey[17], s_ex[17];
  __shared__ unsigned s_cb[256], s_cr[256];
  __shared__ unsigned s_part[2][FS_THREADS / 64];

  const int tid = threadIdx.x;
  const int* j = boxes + 5 * (size_t)blockIdx.x;
  const TmBox p = {j[0], j[1], j[2], j[3], j[4]};
  unsigned char* dst = out + FS_BYTES * (size_t)blockIdx.x;
  // a bad row (block-uniform): read nothing, write zeros
  if (!tm_box_ok(p, nframes, H, W, 16)) {
    dst[tid] = 0;
    if (tid < FS_BYTES - FS_THREADS) dst[FS_THREADS + tid] = 0;
    return;
  }
  const int h = p.bottom - p.top, w = p.right - p.left;
  if (tid <= 16) {
    s_ey[tid] = (int)(((int64_t)tid * h) >> 4);
    s_ex[tid] = (int)(((int64_t)tid * w) >> 4);
  }
  __syncthreads();

  // phase 1: the cell of this thread.  The box lies inside the frame and the cells tile it: no byte outside is read
  const int64_t rs = (int64_t)W * 3;
  const unsigned char* frame = frames + (int64_t)p.f * H * rs;
  const int u = tid >> 4, v = tid & 15;
  unsigned cbs, crs;
  const int c = (int)tm_cell_ycc(frame, rs, p.top + s_ey[u], p.top + s_ey[u + 1], p.left + s_ex[v], p.left + s_ex[v + 1],
                                 cbs, crs);
  s_cb[tid] = cbs;
  s_cr[tid] = crs;

  // phase 2: d = 256 c - S1 is 256 (c - mean) exactly; A = sum |d| <= 256 * 65280 < 2^24
  const int S1 = (int)fs_block_sum((unsigned)c, s_part[0], tid);
  const int d = 256 * c - S1;
  const unsigned ad = (unsigned)(d < 0 ? -d : d);
  const unsigned A = fs_block_sum(ad, s_part[1], tid);
  int nv = 128;
  if (A) {
    const int q = (int)((8192u * ad + A / 2u) / A);                  // 8192 * 65280 + A / 2 < 2^31
    nv = d < 0 ? 128 - q : 128 + q;
    nv = nv < 0 ? 0 : (nv > 255 ? 255 : nv);
  }
  dst[tid] = (unsigned char)nv;

  // phase 3: the chroma cells (s_cb, s_cr are visible: two barriers since they were written)
  if (tid < 128) {
    const int k = tid & 63, cu = k >> 3, cv = k & 7;
    const unsigned* s = tid < 64 ? s_cb : s_cr;
    const int i0 = (2 * cu) * 16 + 2 * cv;
    const unsigned sum = s[i0] + s[i0 + 1] + s[i0 + 16] + s[i0 + 17];
    const unsigned cnt = (unsigned)(s_ey[2 * cu + 2] - s_ey[2 * cu]) * (unsigned)(s_ex[2 * cv + 2] - s_ex[2 * cv]);
    const unsigned m = (sum + cnt / 2u) / cnt;
    dst[FS_THREADS + tid] = (unsigned char)(m > 255u ? 255u : m);    // 256 only where every pixel is (0, 0, 255) or (255, 0, 0)
  }
}

int launch_face_signature(const unsigned char* frames, int nframes, int H, int W, const int* boxes5, int n,
                          unsigned char* out384, hipStream_t s) {
  GCV_REQUIRE(nframes > 0 && H > 0 && W > 0, "face signature: bad geometry");
  // a chroma cell holds fewer than H W / 16 pixels of at most 256 each: its sum is 32 bits
  GCV_REQUIRE((int64_t)H * W <= ((int64_t)1 << 28), "face signature: frames of more than 2^28 pixels");
  GCV_REQUIRE(n >= 0, "face signature: negative box count");
  if (n == 0) return 0;
  hipLaunchKernelGGL(face_signature_kernel, dim3((unsigned)n), dim3(FS_THREADS), 0, s, frames, nframes, H, W, boxes5,
                     out384);
  GCV_CHECK_HIP(hipGetLastError());
  return 0;
}

// ----------------------------------------------------------------------------- gcv_sig_link
constexpr int SL_TILE = 64;                               // rows of a tile
constexpr int SL_THREADS = 256;
constexpr int SL_Q = FS_BYTES / 16;                       // 24 uint4 a row
constexpr int SL_STRIDE_Q = 25;                           // row stride in uint4: 100 dwords (the header comment says why)
constexpr int SL_MAX_ROWS = 65536, SL_MAX_TRACKS = 4096;

// One (owner i, owner j, value) of every lane of the wave into out; called in wave-uniform control flow, all 64 lanes active
__device__ __forceinline__ void sl_emit(unsigned* __restrict__ out, int T, int oa, int ob, unsigned val, int lane) {
  const bool ok = oa >= 0 && ob >= 0 && oa != ob;
  const int key = ok ? oa * T + ob : -1;                  // T <= 4096: below 2^24
  unsigned v = ok ? val : 0xFFFFFFFFu;
#pragma unroll
  for (int m = 1; m < 64; m <<= 1) {
    const unsigned ov = (unsigned)__shfl_xor((int)v, m, 64);
    const int okey = __shfl_xor(key, m, 64);
    if (okey == key) v = ov < v ? ov : v;
  }
  // one key in the whole wave: the butterfly left the wave's minimum in every lane, and lane 0 speaks for all
  const bool uniform = __all(key == __builtin_amdgcn_readfirstlane(key));
  if (ok && (!uniform || lane == 0)) {
    atomicMin(out + (size_t)oa * T + ob, v);
    atomicMin(out + (size_t)ob * T + oa, v);
  }
}

__global__ void __launch_bounds__(SL_THREADS) sig_link_kernel(const uint4* __restrict__ sig, const int* __restrict__ owner,
                                                              int n, int T, unsigned* __restrict__ out) {
  const int I = blockIdx.y, J = blockIdx.x;
  if (J < I) return;                                      // block-uniform
  __shared__ uint4 s_a[SL_TILE * SL_STRIDE_Q], s_b[SL_TILE * SL_STRIDE_Q];
  __shared__ int s_oi[SL_TILE], s_oj[SL_TILE];

  const int tid = threadIdx.x;
  for (int e = tid; e < SL_TILE * SL_Q; e += SL_THREADS) {
    const int r = e / SL_Q, q = e - r * SL_Q;
    const int gi = I * SL_TILE + r, gj = J * SL_TILE + r;
    uint4 va = {0u, 0u, 0u, 0u}, vb = {0u, 0u, 0u, 0u};          // rows past n: zeros, and their owner is -1
    if (gi < n) va = sig[(size_t)gi * SL_Q + q];
    if (gj < n) vb = sig[(size_t)gj * SL_Q + q];
    s_a[r * SL_STRIDE_Q + q] = va;
    s_b[r * SL_STRIDE_Q + q] = vb;
  }
  if (tid < 2 * SL_TILE) {
    const int r = tid & (SL_TILE - 1);
    const int g = (tid < SL_TILE ? I : J) * SL_TILE + r;
    const int o = g < n ? owner[g] : -1;
    (tid < SL_TILE ? s_oi : s_oj)[r] = (o >= 0 && o < T) ? o : -1;       // nothing outside out is ever addressed
  }
  __syncthreads();

  const int ti = tid >> 4, tj = tid & 15;
  unsigned acc[4][4];
#pragma unroll
  for (int x = 0; x < 4; ++x)
#pragma unroll
    for (int y = 0; y < 4; ++y) acc[x][y] = 0u;
#pragma unroll 2
  for (int q = 0; q < SL_Q; ++q) {
    uint4 a[4], b[4];
#pragma unroll
    for (int x = 0; x < 4; ++x) a[x] = s_a[(4 * ti + x) * SL_STRIDE_Q + q];
#pragma unroll
    for (int y = 0; y < 4; ++y) b[y] = s_b[(tj + 16 * y) * SL_STRIDE_Q + q];
#pragma unroll
    for (int x = 0; x < 4; ++x)
#pragma unroll
      for (int y = 0; y < 4; ++y) {
        unsigned s = acc[x][y];
        s = __builtin_amdgcn_sad_u8(a[x].x, b[y].x, s);
        s = __builtin_amdgcn_sad_u8(a[x].y, b[y].y, s);
        s = __builtin_amdgcn_sad_u8(a[x].z, b[y].z, s);
        s = __builtin_amdgcn_sad_u8(a[x].w, b[y].w, s);
        acc[x][y] = s;
      }
  }

  int oi[4], oj[4];
#pragma unroll
  for (int x = 0; x < 4; ++x) oi[x] = s_oi[4 * ti + x];
#pragma unroll
  for (int y = 0; y < 4; ++y) oj[y] = s_oj[tj + 16 * y];
  const int lane = tid & 63;
  if (__all(oi[0] == oi[1] && oi[0] == oi[2] && oi[0] == oi[3])) {       // wave-uniform: every thread's i rows have one owner
#pragma unroll
    for (int y = 0; y < 4; ++y) {
      unsigned m = acc[0][y];
#pragma unroll
      for (int x = 1; x < 4; ++x) m = acc[x][y] < m ? acc[x][y] : m;
      sl_emit(out, T, oi[0], oj[y], m, lane);
    }
  } else {
#pragma unroll
    for (int x = 0; x < 4; ++x)
#pragma unroll
      for (int y = 0; y < 4; ++y) sl_emit(out, T, oi[x], oj[y], acc[x][y], lane);
  }
}

int launch_sig_link(const unsigned char* sig, const int* owner, int n, int T, uint32_t* out, hipStream_t s) {
  GCV_REQUIRE(n >= 0 && n <= SL_MAX_ROWS, "sig link: n outside 0 ... 65536");
  GCV_REQUIRE(T >= 0 && T <= SL_MAX_TRACKS, "sig link: T outside 0 ... 4096");
  if (n == 0 || T == 0) return 0;
  GCV_REQUIRE(((uintptr_t)sig & 15u) == 0, "sig link: sig must be 16-byte aligned");
  GCV_CHECK_HIP(hipMemsetAsync(out, 0xFF, (size_t)T * T * sizeof(uint32_t), s));
  const unsigned tiles = (unsigned)((n + SL_TILE - 1) / SL_TILE);
  hipLaunchKernelGGL(sig_link_kernel, dim3(tiles, tiles), dim3(SL_THREADS), 0, s, reinterpret_cast<const uint4*>(sig),
                     owner, n, T, out);
  GCV_CHECK_HIP(hipGetLastError());
  return 0;
}

}  // namespace gcv
