// The decoder's and the encoder's side of the scan: YUV 4:2:0 frames (planar I420 or semi-planar NV12, 1.5 bytes a pixel)
// to the uint8 RGB slab every other scan kernel reads, and an RGB slab back to YUV 4:2:0 (gcv_yuv420_to_rgb,
// gcv_rgb_to_yuv420, include/genconvit_hip.h).  Both are pure streaming kernels: 1.5 bytes in and 3 out per pixel, or the
// reverse, every byte touched once, no LDS.
//
// The walk: one thread owns a 2 x 8 patch — two rows of a run of 8 pixels, which is the 4 chroma samples of that run.
// Each chroma sample is therefore read (or written) by one thread, once.  Consecutive lanes take consecutive runs of a
// row pair, so a wave reads 512 consecutive bytes of each of the two Y rows and 256 of chroma, and writes 1536
// consecutive bytes of each RGB row.
//   fast path  W % 8 == 0 and both pointers 8-byte aligned (720p, 1080p): a frame then starts at a multiple of 8 bytes
//              (3 H W / 2 with H even), and so does every patch row — Y rows are one dwordx2 each, chroma one dwordx2
//              (nv12) or two dwords (i420), and an RGB row of the patch is 24 bytes at a multiple of 24: three dwordx2.
//              annotate.hip's 12-byte pieces of 4 pixels are these halved; 8 pixels are the widest run whose RGB stays
//              8-byte aligned for every W % 8 == 0, and 16-byte accesses would want W % 16 == 0 and leave half the lanes
//              of a narrow frame idle.
//   any path   any even W and any alignment (frames packed back to back start at f 3 H W / 2, odd multiples of 2 for
//              many small sizes): the same patch byte by byte, the last run of a row holding W % 8 pixels.
// Both paths fill the same registers and share the arithmetic, which is all-integer and fixed by the header, so that
// tests/yuvutil.py restates it bit for bit.  The four coefficient tables (2 matrices x 2 ranges) are the literals below:
// round(c 2^14) of the real coefficients, derived in exact fractions in tests/yuvutil.py.
#include <cstdint>

#include "common.h"

namespace gcv {

constexpr int YUV_THREADS = 256;
constexpr int YUV_RUN = 8;        // pixels a thread owns of each of its two rows

// R = cy y' + crv v', G = cy y' + cgu u' + cgv v', B = cy y' + cbu u'  (x 2^14), y' = Y - oy
struct YuvIn { int oy, cy, crv, cgu, cgv, cbu; };
// Y = oy + (ar R + ag G + ab B) (x 2^14); U, V from the block sums (x 2^16)
struct YuvOut { int oy, ar, ag, ab, ur, ug, ub, vr, vg, vb; };

// index: matrix * 2 + full_range; matrix 0 = bt601, 1 = bt709
constexpr YuvIn YUV_IN[4] = {{16, 19077, 26149, -6419, -13320, 33050},
                             {0, 16384, 22970, -5638, -11700, 29032},
                             {16, 19077, 29372, -3494, -8731, 34610},
                             {0, 16384, 25802, -3069, -7670, 30402}};
constexpr YuvOut YUV_OUT[4] = {{16, 4207, 8260, 1604, -2428, -4768, 7196, 7196, -6026, -1170},
                               {0, 4899, 9617, 1868, -2765, -5427, 8192, 8192, -6860, -1332},
                               {16, 2991, 10064, 1016, -1649, -5547, 7196, 7196, -6536, -660},
                               {0, 3483, 11718, 1183, -1877, -6315, 8192, 8192, -7441, -751}};

struct alignas(8) YuvPair { uint32_t w[2]; };

// the patch a thread owns: frame, row pair, first column, and how many of the run's pixels exist (even, 2 ... 8)
struct YuvPatch { size_t f; unsigned yy, x0; int np; };

__device__ __forceinline__ bool yuv_patch(unsigned items, int H, int W, YuvPatch& p) {
  const unsigned i = blockIdx.x * (unsigned)YUV_THREADS + threadIdx.x;
  if (i >= items) return false;
  const unsigned runs = ((unsigned)W + YUV_RUN - 1) / YUV_RUN, per = ((unsigned)H >> 1) * runs;
  const unsigned f = i / per, r = i - f * per;
  p.f = f;
  p.yy = r / runs;
  p.x0 = (r - p.yy * runs) * YUV_RUN;
  p.np = min(YUV_RUN, W - (int)p.x0);
  return true;
}

__device__ __forceinline__ int yuv_byte(const uint32_t* w, int i) { return (int)(w[i >> 2] >> (8 * (i & 3)) & 255u); }

// n bytes (n <= 4 NW, known only at run time) into NW zeroed words, and back
template <int NW>
__device__ __forceinline__ void yuv_load_bytes(uint32_t (&w)[NW], const unsigned char* src, int n) {
#pragma unroll
  for (int k = 0; k < NW; ++k) w[k] = 0;
#pragma unroll
  for (int i = 0; i < 4 * NW; ++i)
    if (i < n) w[i >> 2] |= (uint32_t)src[i] << (8 * (i & 3));
}

template <int NW>
__device__ __forceinline__ void yuv_store_bytes(unsigned char* dst, const uint32_t (&w)[NW], int n) {
#pragma unroll
  for (int i = 0; i < 4 * NW; ++i)
    if (i < n) dst[i] = (unsigned char)(w[i >> 2] >> (8 * (i & 3)));
}

template <int NW>
__device__ __forceinline__ void yuv_load_pairs(uint32_t (&w)[NW], const unsigned char* src) {
#pragma unroll
  for (int k = 0; k < NW; k += 2) {
    const YuvPair v = *reinterpret_cast<const YuvPair*>(src + 4 * k);
    w[k] = v.w[0]; w[k + 1] = v.w[1];
  }
}

template <int NW>
__device__ __forceinline__ void yuv_store_pairs(unsigned char* dst, const uint32_t (&w)[NW]) {
#pragma unroll
  for (int k = 0; k < NW; k += 2) {
    YuvPair v;
    v.w[0] = w[k]; v.w[1] = w[k + 1];
    *reinterpret_cast<YuvPair*>(dst + 4 * k) = v;
  }
}

__device__ __forceinline__ uint32_t yuv_clip(int v) { return (uint32_t)min(max(v, 0), 255); }

// clip(v >> 14, 0, 255), with the clip taken before the shift: the two are the same value (both steps are monotone and
// 255 << 14 | 16383 is the largest v that shifts to 255).  Written the other way round, hipcc (ROCm 7.2) fuses two such
// channels into one v_ashr_pk_u8_i32 and ORs its result into the packed word as if bits 16 ... 31 were zero; on the
// MI355X they are not, and a channel that saturates spills into the byte after its pair (seen as wrong B / R bytes
// against tests/yuvutil.py).  The build's report refuses the instruction in this file (isa_report.py).
__device__ __forceinline__ uint32_t yuv_clip14(int v) { return (uint32_t)(min(max(v, 0), (255 << 14) | 16383) >> 14); }

template <bool VEC, bool NV12>
__global__ void __launch_bounds__(YUV_THREADS) yuv420_to_rgb_kernel(const unsigned char* __restrict__ yuv, unsigned items,
                                                                    int H, int W, YuvIn k, unsigned char* __restrict__ rgb) {
  YuvPatch p;
  if (!yuv_patch(items, H, W, p)) return;
  const size_t HW = (size_t)H * (size_t)W;
  const unsigned char* frame = yuv + p.f * (HW + HW / 2);
  const unsigned char* ysrc = frame + (size_t)(2 * p.yy) * W + p.x0;
  uint32_t ya[2], yb[2], ca[2], cb[1];                   // two Y rows; chroma: nv12 8 bytes U V U V ..., i420 4 of U and 4 of V
  if (NV12) {
    const unsigned char* c = frame + HW + (size_t)p.yy * W + p.x0;
    if (VEC) yuv_load_pairs(ca, c); else yuv_load_bytes(ca, c, p.np);
    cb[0] = 0;
  } else {
    const unsigned char* u = frame + HW + (size_t)p.yy * (W >> 1) + (p.x0 >> 1);
    const unsigned char* v = u + HW / 4;
    uint32_t one[1];
    if (VEC) {
      ca[0] = *reinterpret_cast<const uint32_t*>(u);
      cb[0] = *reinterpret_cast<const uint32_t*>(v);
    } else {
      yuv_load_bytes(one, u, p.np >> 1); ca[0] = one[0];
      yuv_load_bytes(one, v, p.np >> 1); cb[0] = one[0];
    }
    ca[1] = 0;
  }
  if (VEC) { yuv_load_pairs(ya, ysrc); yuv_load_pairs(yb, ysrc + W); }
  else { yuv_load_bytes(ya, ysrc, p.np); yuv_load_bytes(yb, ysrc + W, p.np); }

  uint32_t ra[6] = {0, 0, 0, 0, 0, 0}, rb[6] = {0, 0, 0, 0, 0, 0};   // the two RGB rows of the patch, 24 bytes each
#pragma unroll
  for (int j = 0; j < YUV_RUN / 2; ++j) {                // one chroma sample: a 2 x 2 block
    const int u = (NV12 ? yuv_byte(ca, 2 * j) : yuv_byte(ca, j)) - 128;
    const int v = (NV12 ? yuv_byte(ca, 2 * j + 1) : yuv_byte(cb, j)) - 128;
    const int dr = k.crv * v + 8192, dg = k.cgu * u + k.cgv * v + 8192, db = k.cbu * u + 8192;
#pragma unroll
    for (int q = 0; q < 2; ++q) {
      const int px = 2 * j + q;
      const int la = k.cy * (yuv_byte(ya, px) - k.oy), lb = k.cy * (yuv_byte(yb, px) - k.oy);
      const uint32_t a[3] = {yuv_clip14(la + dr), yuv_clip14(la + dg), yuv_clip14(la + db)};
      const uint32_t b[3] = {yuv_clip14(lb + dr), yuv_clip14(lb + dg), yuv_clip14(lb + db)};
#pragma unroll
      for (int c = 0; c < 3; ++c) {
        const int at = 3 * px + c;
        ra[at >> 2] |= a[c] << (8 * (at & 3));
        rb[at >> 2] |= b[c] << (8 * (at & 3));
      }
    }
  }
  unsigned char* dst = rgb + (p.f * HW + (size_t)(2 * p.yy) * W + p.x0) * 3;
  if (VEC) { yuv_store_pairs(dst, ra); yuv_store_pairs(dst + (size_t)W * 3, rb); }
  else { yuv_store_bytes(dst, ra, 3 * p.np); yuv_store_bytes(dst + (size_t)W * 3, rb, 3 * p.np); }
}

template <bool VEC, bool NV12>
__global__ void __launch_bounds__(YUV_THREADS) rgb_to_yuv420_kernel(const unsigned char* __restrict__ rgb, unsigned items,
                                                                    int H, int W, YuvOut k, unsigned char* __restrict__ yuv) {
  YuvPatch p;
  if (!yuv_patch(items, H, W, p)) return;
  const size_t HW = (size_t)H * (size_t)W;
  const unsigned char* src = rgb + (p.f * HW + (size_t)(2 * p.yy) * W + p.x0) * 3;
  uint32_t ra[6], rb[6];
  if (VEC) { yuv_load_pairs(ra, src); yuv_load_pairs(rb, src + (size_t)W * 3); }
  else { yuv_load_bytes(ra, src, 3 * p.np); yuv_load_bytes(rb, src + (size_t)W * 3, 3 * p.np); }

  uint32_t ya[2] = {0, 0}, yb[2] = {0, 0}, ca[2] = {0, 0}, cb[1] = {0};
#pragma unroll
  for (int j = 0; j < YUV_RUN / 2; ++j) {
    int sr = 0, sg = 0, sb = 0;                          // the block's sums, 0 ... 1020
#pragma unroll
    for (int q = 0; q < 2; ++q) {
      const int px = 2 * j + q;
      const int r0 = yuv_byte(ra, 3 * px), g0 = yuv_byte(ra, 3 * px + 1), b0 = yuv_byte(ra, 3 * px + 2);
      const int r1 = yuv_byte(rb, 3 * px), g1 = yuv_byte(rb, 3 * px + 1), b1 = yuv_byte(rb, 3 * px + 2);
      ya[px >> 2] |= (uint32_t)(k.oy + ((k.ar * r0 + k.ag * g0 + k.ab * b0 + 8192) >> 14)) << (8 * (px & 3));
      yb[px >> 2] |= (uint32_t)(k.oy + ((k.ar * r1 + k.ag * g1 + k.ab * b1 + 8192) >> 14)) << (8 * (px & 3));
      sr += r0 + r1; sg += g0 + g1; sb += b0 + b1;
    }
    const uint32_t u = yuv_clip(128 + ((k.ur * sr + k.ug * sg + k.ub * sb + 32768) >> 16));
    const uint32_t v = yuv_clip(128 + ((k.vr * sr + k.vg * sg + k.vb * sb + 32768) >> 16));
    if (NV12) {
      ca[j >> 1] |= (u | v << 8) << (16 * (j & 1));
    } else {
      ca[0] |= u << (8 * j);
      cb[0] |= v << (8 * j);
    }
  }
  unsigned char* frame = yuv + p.f * (HW + HW / 2);
  unsigned char* ydst = frame + (size_t)(2 * p.yy) * W + p.x0;
  if (VEC) { yuv_store_pairs(ydst, ya); yuv_store_pairs(ydst + W, yb); }
  else { yuv_store_bytes(ydst, ya, p.np); yuv_store_bytes(ydst + W, yb, p.np); }
  if (NV12) {
    unsigned char* c = frame + HW + (size_t)p.yy * W + p.x0;
    if (VEC) yuv_store_pairs(c, ca); else yuv_store_bytes(c, ca, p.np);
  } else {
    unsigned char* u = frame + HW + (size_t)p.yy * (W >> 1) + (p.x0 >> 1);
    unsigned char* v = u + HW / 4;
    if (VEC) {
      *reinterpret_cast<uint32_t*>(u) = ca[0];
      *reinterpret_cast<uint32_t*>(v) = cb[0];
    } else {
      const uint32_t one_u[1] = {ca[0]}, one_v[1] = {cb[0]};
      yuv_store_bytes(u, one_u, p.np >> 1);
      yuv_store_bytes(v, one_v, p.np >> 1);
    }
  }
}

// the checks both entries share; *items is the number of 2 x 8 patches, 0 when there is nothing to launch
static int yuv_check(const void* in, const void* out, int nframes, int H, int W, int layout, int matrix, unsigned* items) {
  GCV_REQUIRE(H >= 2 && W >= 2 && H % 2 == 0 && W % 2 == 0 && H <= 65536 && W <= 65536, "yuv420: H and W must be even, 2 ... 65536");
  GCV_REQUIRE(layout == 0 || layout == 1, "yuv420: layout must be 0 (i420) or 1 (nv12)");
  GCV_REQUIRE(matrix == 0 || matrix == 1, "yuv420: matrix must be 0 (bt601) or 1 (bt709)");
  GCV_REQUIRE(nframes >= 0, "yuv420: negative frame count");
  GCV_REQUIRE((int64_t)nframes * H * W < ((int64_t)1 << 31), "yuv420: too many pixels for one launch");
  GCV_REQUIRE(nframes == 0 || (in && out), "yuv420: null pointer");
  *items = (unsigned)nframes * ((unsigned)H >> 1) * (((unsigned)W + YUV_RUN - 1) / YUV_RUN);   // <= nframes H W / 4 < 2^29
  return 0;
}

#define YUV_LAUNCH(KERNEL, VEC, NV12, ...) \
  hipLaunchKernelGGL((KERNEL<VEC, NV12>), dim3((items + YUV_THREADS - 1) / YUV_THREADS), dim3(YUV_THREADS), 0, s, __VA_ARGS__)
#define YUV_DISPATCH(KERNEL, ...)                                         \
  do {                                                                    \
    if (vec && layout) YUV_LAUNCH(KERNEL, true, true, __VA_ARGS__);       \
    else if (vec) YUV_LAUNCH(KERNEL, true, false, __VA_ARGS__);           \
    else if (layout) YUV_LAUNCH(KERNEL, false, true, __VA_ARGS__);        \
    else YUV_LAUNCH(KERNEL, false, false, __VA_ARGS__);                   \
  } while (0)

int launch_yuv420_to_rgb(const unsigned char* yuv, int nframes, int H, int W, int layout, int matrix, int full_range,
                         unsigned char* rgb, hipStream_t s) {
  unsigned items = 0;
  if (int rc = yuv_check(yuv, rgb, nframes, H, W, layout, matrix, &items)) return rc;
  if (items == 0) return 0;
  const bool vec = W % YUV_RUN == 0 && (((uintptr_t)yuv | (uintptr_t)rgb) & 7u) == 0;
  const YuvIn k = YUV_IN[matrix * 2 + (full_range ? 1 : 0)];
  YUV_DISPATCH(yuv420_to_rgb_kernel, yuv, items, H, W, k, rgb);
  GCV_CHECK_HIP(hipGetLastError());
  return 0;
}

int launch_rgb_to_yuv420(const unsigned char* rgb, int nframes, int H, int W, int layout, int matrix, int full_range,
                         unsigned char* yuv, hipStream_t s) {
  unsigned items = 0;
  if (int rc = yuv_check(rgb, yuv, nframes, H, W, layout, matrix, &items)) return rc;
  if (items == 0) return 0;
  const bool vec = W % YUV_RUN == 0 && (((uintptr_t)yuv | (uintptr_t)rgb) & 7u) == 0;
  const YuvOut k = YUV_OUT[matrix * 2 + (full_range ? 1 : 0)];
  YUV_DISPATCH(rgb_to_yuv420_kernel, rgb, items, H, W, k, yuv);
  GCV_CHECK_HIP(hipGetLastError());
  return 0;
}

}  // namespace gcv
