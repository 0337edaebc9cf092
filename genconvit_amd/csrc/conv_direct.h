// Direct 3x3 convolution for 16-bit storage at Cin = 16 / 32 and N = 32 / 64 (ED encoder layers 2-3: conv + ReLU + 2x2
// max-pool; VAE encoder layers 2-3: conv stride 2 + LeakyReLU).  One of the three kinds of kernel that gemm_select
// (gemm_impl.h) picks from: the A_IM2COL3_POOL / EPI_POOL4 and A_IM2COL3_S2 / EPI_BIAS_ACT launches that meet its rules there
// run here, everything else stays on gemm_kernel.
//
// Why: at these widths a wave of gemm_kernel issues 2-4 MFMAs per K tile and pays gathered loads with tap / bounds / address
// arithmetic, an LDS store, an LDS read-back and a barrier for each of them.  Here both MFMA operands come straight from
// memory and there is no LDS and no barrier at all:
//   * a wave's work item is 32 conv pixels (32 consecutive rows m of the flattened launch, in the launch's own row order,
//     so a block may straddle image rows and images and there is no rule on the width) x one block of 32 output channels;
//   * the weights of that channel block are 9 * Cin / 16 MFMA A fragments (36 / 72 registers), loaded once per wave;  at
//     N = 64 the two channel blocks belong to two neighbouring waves, which read the same pixels through L1;
//   * the B fragment of k-step (tap, half) is ONE 16-byte global load per lane: channels 16 half + 8 (lane >> 5) .. + 7 of
//     the lane's pixel shifted by the tap.  The fragments of the wave's next pixel block are loaded into the registers of
//     the current one as its MFMAs release them (each load is issued beside the MFMA that consumed its register);
//   * a tap that falls outside the image (or a lane past M) loads from the lane's own centre pixel - never from an address
//     outside the tensor - and the fragment is then masked to zero.
//
// Every output bit is the one gemm_kernel produces:
//   * the same Mfma<T>::run(W fragment, pixel fragment, acc) (v_mfma_f32_32x32x16, W as the A operand), acc starting at 0,
//     k-steps in ascending k = tap * Cin + ci on one accumulation chain.  gemm_kernel pads K = 144 to 160 with zero
//     operands; those steps add +0 and change nothing (an accumulator that starts at +0 never becomes -0).  Which lane
//     carries which pixel does not enter the sum: a column of the MFMA is one pixel's dot product;
//   * the bias is added AFTER the chain by the same bias_act4 (not preloaded into the accumulator), then from_f<T>;
//   * pool mode: gemm_kernel computes  from_f(max_4(to_f(from_f(relu(acc + bias))))).  x -> x + bias, ReLU and the
//     rounding are monotone non-decreasing, so they commute with max bit for bit; here the 2x2 max is taken first, so
//     bias, ReLU and the conversion run on a quarter of the values.
// profiles/enc_conv_direct_bits.py compares the two on the network's shapes with np.array_equal.
#pragma once
#include <algorithm>

#include "gemm.h"

namespace gcv {

struct ConvDirectArgs {
  const void* x;        // NHWC input (nimg, H, W, Cin)
  const void* wt;       // (N, 9 * Cin), k = tap * Cin + ci
  void* out;
  const float* bias;    // (N)
  int M, N, ldc;
  int H, W;
  int nblk;             // 32-row pixel blocks
  uint32_t mg_w, mg_h;  // floor(2^32 / (W / 2)), floor(2^32 / (H / 2))  (2^32 - 1 for a divisor of 1)
};

// p / d for any 32-bit p: mg = floor(2^32 / d) under-estimates the quotient by at most one
__device__ __forceinline__ uint32_t udiv_mg(uint32_t p, uint32_t d, uint32_t mg, uint32_t& rem) {
  uint32_t q = __umulhi(p, mg);
  uint32_t r = p - q * d;
  if (r >= d) { ++q; r -= d; }
  rem = r;
  return q;
}
static inline uint32_t udiv_mg_of(uint32_t d) { return d <= 1 ? 0xffffffffu : (uint32_t)((1ull << 32) / d); }

// STRIDE 1: rows m = window * 4 + (dy * 2 + dx), ReLU, 2x2 max-pool, output row m >> 2 (EPI_POOL4)
// STRIDE 2: rows m = output pixel, input centre (2 yo, 2 xo), LeakyReLU (EPI_BIAS_ACT)
template <typename T, int CIN, int STRIDE>
__global__ void __launch_bounds__(256, 2) conv3_direct_kernel(const ConvDirectArgs a) {
  static_assert(sizeof(T) == 2 && (CIN == 16 || CIN == 32) && (STRIDE == 1 || STRIDE == 2), "16-bit storage, Cin 16 / 32");
  constexpr int HALVES = CIN / 16;
  constexpr int KS = 9 * HALVES;                // k-steps of 16
  constexpr int PIXB = CIN * 2;                 // bytes per pixel
  const int lane = threadIdx.x & 63;
  const int lr = lane & 31, lh = lane >> 5;
  // Row of the block that MFMA column lr carries.  Stride 2: lr itself.  Pool mode: column (rho = lr >> 4, i = lr & 15)
  // carries row 4 (i >> 1) + 2 rho + (i & 1), i.e. window i >> 1, dy = rho, dx = i & 1: four consecutive lanes then read
  // four horizontally consecutive pixels instead of a 2x2 window's two image rows.  The L1 takes a wave's load a lane quad
  // at a time and the time follows the 64-byte pieces a quad touches: 2-3 instead of 2-4 at Cin = 16, 37.6 -> 28.5 us for
  // the 16 -> 32 layer at 128 frames (always 4 at Cin = 32, where a pixel is 64 bytes: 38.8 -> 37.1).  A pool window is
  // then lanes {2 w, 2 w + 1} of two neighbouring 16-lane rows.
  const int ml = STRIDE == 1 ? (((lr & 15) >> 1) << 2) + ((lr >> 4) << 1) + (lr & 1) : lr;
  const int ncb = a.N >> 5;                     // 1 or 2 channel blocks
  const int gw = blockIdx.x * 4 + __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int cb = gw & (ncb - 1);
  const int wv = gw / ncb, nwv = (int)(gridDim.x * 4) / ncb;
  if (wv >= a.nblk) return;

  const unsigned char* const xb = (const unsigned char*)a.x;
  const int H = a.H, W = a.W;
  const uint32_t Ho = (uint32_t)H >> 1, Wo = (uint32_t)W >> 1;

  // weights of this channel block: lane (channel lr, half lh) holds k = 16 s + 8 lh .. + 7 of k-step s
  u32x4 wf[KS];
  {
    const T* wp = (const T*)a.wt + (size_t)(cb * 32 + lr) * (9 * CIN) + 8 * lh;
#pragma unroll
    for (int s = 0; s < KS; ++s) wf[s] = *(const u32x4*)(wp + 16 * s);
  }

  // byte offset of the lane's centre pixel (+ its channel half) and the 9-bit mask of taps inside the image; lanes past M
  // take the last row's pixel and an empty mask
  auto setup = [&](int pb, uint32_t& off, uint32_t& vm) {
    const int m = pb * 32 + ml;
    const uint32_t mc = (uint32_t)min(m, a.M - 1);
    uint32_t xo, yo;
    const uint32_t p = STRIDE == 1 ? mc >> 2 : mc;
    const uint32_t t = udiv_mg(p, Wo, a.mg_w, xo);
    const uint32_t b = udiv_mg(t, Ho, a.mg_h, yo);
    const int y = 2 * (int)yo + (STRIDE == 1 ? (int)((mc >> 1) & 1) : 0);
    const int x = 2 * (int)xo + (STRIDE == 1 ? (int)(mc & 1) : 0);
    off = ((b * (uint32_t)H + (uint32_t)y) * (uint32_t)W + (uint32_t)x) * PIXB + 16 * lh;
    const uint32_t cm = (x >= 1 ? 1u : 0u) | 2u | (x + 1 < W ? 4u : 0u);
    uint32_t v = cm << 3;
    if (y >= 1) v |= cm;
    if (y + 1 < H) v |= cm << 6;
    vm = m < a.M ? v : 0u;
  };
  auto load = [&](uint32_t off, uint32_t vm, int s) {
    const int tap = s / HALVES, half = s % HALVES;
    const int ky = tap / 3, kx = tap % 3;
    const int delta = ((ky - 1) * W + (kx - 1)) * PIXB;
    const uint32_t o = ((vm >> tap) & 1u) ? off + (uint32_t)delta : off;       // clamped: always inside the tensor
    return *(const u32x4*)(xb + (size_t)o + 32 * half);
  };

  // bias of the channels this lane finishes
  const float* const bp = a.bias + cb * 32 + 4 * lh;
  f32x4 bq[STRIDE == 1 ? 1 : 4];
  const int grp = 2 * ((lane >> 4) & 1) + (lane & 1);        // pool mode: the channel group (of 8) this lane finishes
  if (STRIDE == 1) {
    bq[0] = *(const f32x4*)(bp + 8 * grp);
  } else {
#pragma unroll
    for (int q = 0; q < 4; ++q) bq[STRIDE == 1 ? 0 : q] = *(const f32x4*)(bp + 8 * q);
  }

  T* const op = (T*)a.out + cb * 32;
  typedef T t2 __attribute__((ext_vector_type(2)));
  typedef T t4 __attribute__((ext_vector_type(4)));

  uint32_t off_c, vm_c;
  setup(wv, off_c, vm_c);
  u32x4 fr[KS];
#pragma unroll
  for (int s = 0; s < KS; ++s) {
    fr[s] = load(off_c, vm_c, s);
    __builtin_amdgcn_sched_barrier(0);          // issue order = use order, as in the loop: the first wait is vmcnt(KS - 1)
  }

  for (int pb = wv; pb < a.nblk; pb += nwv) {
    // the next block's fragments; behind the last block every lane re-reads one line of the tensor's first pixel
    uint32_t off_n = 16 * lh, vm_n = 0u;
    if (pb + nwv < a.nblk) setup(pb + nwv, off_n, vm_n);

    f32x16 acc;
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[r] = 0.0f;
#pragma unroll
    for (int s = 0; s < KS; ++s) {
      const uint32_t keep = (uint32_t)(((int)(vm_c << (31 - s / HALVES))) >> 31);     // all ones: tap inside the image
      const u32x4 pf = {fr[s][0] & keep, fr[s][1] & keep, fr[s][2] & keep, fr[s][3] & keep};
      Mfma<T>::run(wf[s], pf, acc);
      fr[s] = load(off_n, vm_n, s);
      // keep the load behind its MFMA: left alone, hipcc sinks all of a block's loads below its last MFMA and waits for
      // them with vmcnt(0) in front of the next block's first one
      __builtin_amdgcn_sched_barrier(0);
    }

    const int m = pb * 32 + ml;
    if constexpr (STRIDE == 1) {
      // acc[4 q + e]: column lr, channel 8 q + 4 lh + e.  v_permlane16_swap exchanges the odd 16-lane rows of its first
      // operand with the even rows of its second: of (acc[4 q + e], acc[4 (q + 2) + e]) the even rows (dy = 0) then hold
      // both image rows of channel group q and the odd rows (dy = 1) those of group q + 2 - one maximum each, and one more
      // with the dx neighbour (DPP quad_perm [1,0,3,2]).  The window's lane (dy, dx) finishes group 2 dy + dx: 8 bytes
      // per lane, the wave's 64 lanes cover 8 windows x 32 channels = 512 contiguous bytes at N = 32.
      float v[4];
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        float t[2];
#pragma unroll
        for (int q = 0; q < 2; ++q) {
          const float lo = acc[4 * q + e], hi = acc[4 * (q + 2) + e];
          const auto sw = __builtin_amdgcn_permlane16_swap(__builtin_bit_cast(uint32_t, lo), __builtin_bit_cast(uint32_t, hi),
                                                           false, false);
          const float u = fmaxf(__builtin_bit_cast(float, (uint32_t)sw[0]), __builtin_bit_cast(float, (uint32_t)sw[1]));
          t[q] = fmaxf(u, GCV_DPP_F32(u, 0xB1));
        }
        v[e] = (lane & 1) ? t[1] : t[0];
      }
      bias_act4<ACT_RELU, T>(v, bq[0]);
      const t4 o4 = {from_f<T>(v[0]), from_f<T>(v[1]), from_f<T>(v[2]), from_f<T>(v[3])};
      if (m < a.M) *(t4*)(op + (int64_t)(m >> 2) * a.ldc + 8 * grp + 4 * lh) = o4;
    } else {
      uint2 pk[4];
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        float v[4];
#pragma unroll
        for (int e = 0; e < 4; ++e) v[e] = acc[4 * q + e];
        bias_act4<ACT_LEAKY, T>(v, bq[STRIDE == 1 ? 0 : q]);
        pk[q].x = __builtin_bit_cast(uint32_t, (t2){from_f<T>(v[0]), from_f<T>(v[1])});
        pk[q].y = __builtin_bit_cast(uint32_t, (t2){from_f<T>(v[2]), from_f<T>(v[3])});
      }
      // one v_permlane32_swap per dword of a (q, q + 1) pair: lanes 0-31 get the 16 bytes of piece q (channels 8 q .. + 7),
      // lanes 32-63 those of piece q + 1
#pragma unroll
      for (int pp = 0; pp < 2; ++pp) {
        const auto sx = __builtin_amdgcn_permlane32_swap(pk[2 * pp].x, pk[2 * pp + 1].x, false, false);
        const auto sy = __builtin_amdgcn_permlane32_swap(pk[2 * pp].y, pk[2 * pp + 1].y, false, false);
        const u32x4 w = {sx[0], sy[0], sx[1], sy[1]};
        if (m < a.M) *(u32x4*)(op + (int64_t)m * a.ldc + 8 * (2 * pp + lh)) = w;
      }
    }
    off_c = off_n;
    vm_c = vm_n;
  }
}

// Which launches take the direct kernel: bit 0 pool Cin = 16, bit 1 pool Cin = 32, bit 2 stride 2 Cin = 16, bit 3 stride 2
// Cin = 32.  All four instances are bit-identical to gemm_kernel; the default is what measured faster on the MI355X
// (DESIGN.md 4.1), other values are for A/B builds (0: every im2col launch on gemm_kernel).
#ifndef GCV_CONV_DIRECT
#define GCV_CONV_DIRECT 7
#endif
constexpr bool conv_direct_on(bool pool, int cin) { return (GCV_CONV_DIRECT >> ((pool ? 0 : 2) + (cin == 32 ? 1 : 0))) & 1; }

// at most four workgroups per CU of a 256-CU chip are launched (the grid is planned with the kernel: gemm_select, gemm_impl.h)
constexpr int kConvDirectMaxWg = 1024;

static inline ConvDirectArgs conv_direct_args(const GemmArgs& g) {
  ConvDirectArgs a;
  a.x = g.A; a.wt = g.Wt; a.out = g.C; a.bias = g.bias;
  a.M = g.M; a.N = g.N; a.ldc = g.ldc; a.H = g.H; a.W = g.W;
  a.nblk = cdiv(g.M, 32);
  a.mg_w = udiv_mg_of((uint32_t)g.W >> 1);
  a.mg_h = udiv_mg_of((uint32_t)g.H >> 1);
  return a;
}

}  // namespace gcv
