// Fused ConvNeXt MLP, C = 96, weights RESIDENT in LDS (16-bit storage):
//     out = resid + gamma * ( W2 . GELU( W1 . x_ln + b1 ) + b2 )
//
// Why a second kernel for the first stage: at C = 96 the MLP is bound by the GELU, not by the MFMAs (per 32-token
// wave tile: 144 MFMAs = 4.6k matrix cycles against ~2.9k VALU instructions = 11.5k issue cycles), so the only
// way to finish sooner is to keep the vector pipe issuing all the time.  fused_mlp_kernel streams the weights
// through LDS in chunks, which costs a workgroup barrier per chunk; the barrier puts every wave of the CU in the
// same phase (all in GEMM1, then all in GELU, then all in GEMM2), so matrix and vector work never overlap.
// Here both weight matrices (2 x 73.7 KB as 16-bit) live in LDS for the whole kernel:
//   * one persistent 8-wave workgroup per CU loads W1 / W2 / b1 / b2 / gamma once (150 KB of the 160 KB LDS) and then
//     never synchronises again: each wave walks its own 32-token tiles, so the two waves of a SIMD drift apart and one
//     wave's GELU issues under the other's MFMAs
//   * inside a wave the work is software-pipelined over 32-wide hidden groups g: GEMM1(g+1) and GEMM2(g-1) (12
//     independent MFMAs) are issued around GELU(g), so its own vector instructions also have matrix work to hide under
//   * rows are 192 B (no room for padding): the 16-byte chunk index is XOR-swizzled inside groups of four by
//     (row >> 2) & 3, which puts the 16 lanes of a ds_read_b128 group on 16 distinct 16-byte bank groups
//   * no LDS is left for an epilogue transposition: a v_permlane32_swap per dword pairs the two half-waves' 8-byte
//     halves of the (token on lane, 4 channels in registers) accumulator, which is stored as 16-byte pieces, 32 rows
//     x 32 B per instruction; L2 merges the 6 pieces of a row before write-back
#pragma once
#include "fused_mlp.h"

namespace gcv {

struct MlpResSmem {
  static constexpr int kRow = 192;                       // bytes per row of either weight image (96 x 16-bit)
  static constexpr int kW1 = 0;                          // [384 hidden][96 k]
  static constexpr int kW2 = 384 * kRow;                 // [4 chunks][96 out][96 hidden (permuted)]
  static constexpr int kB1 = 2 * 384 * kRow;             // 384 floats
  static constexpr int kB2 = kB1 + 384 * 4;              // 96 floats
  static constexpr int kG = kB2 + 96 * 4;                // 96 floats
  static constexpr int kCtr = kG + 96 * 4;               // tile counter of the workgroup (one dword)
  static constexpr int kLn = kCtr + 16;                  // LNP variant: LayerNorm weight | bias of the stage boundary (2 x 96 floats)
  static constexpr int bytes = kLn + 2 * 96 * 4;         // 150544
};

__device__ __forceinline__ int mlp_res_swz(int row, int k16) { return (k16 & ~3) | ((k16 & 3) ^ ((row >> 2) & 3)); }

// LNP: the epilogue applies the stage boundary's LayerNorm2d + 2x2 space-to-depth instead of storing the residual stream
// (MlpArgs::lnp): a wave owns whole token rows (lanes l and l + 32 hold the two halves of a row's 96 channels), so the
// statistics are 96 register operations and one cross-lane exchange, and LN-patchify's pass over the tensor (77 MB read +
// 77 MB written per 128 images) disappears together with this kernel's own 77 MB store.
template <typename T, bool LNP = false>
__global__ void __launch_bounds__(512, 1) fused_mlp_res_kernel(const MlpArgs a) {
  static_assert(sizeof(T) == 2, "fused MLP is built for 16-bit storage");
  constexpr int C = 96, HC = 96, NG = 12;                 // 12 hidden groups of 32
  constexpr int KP1 = C / 16;                             // 6 k-steps of GEMM1
  constexpr int NO = C / 32;                              // 3 output-channel tiles
  constexpr int ROW = MlpResSmem::kRow;
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  const unsigned char* sW1 = smem + MlpResSmem::kW1;
  const unsigned char* sW2 = smem + MlpResSmem::kW2;
  const float* sB1 = reinterpret_cast<const float*>(smem + MlpResSmem::kB1);
  const float* sB2 = reinterpret_cast<const float*>(smem + MlpResSmem::kB2);
  const float* sG = reinterpret_cast<const float*>(smem + MlpResSmem::kG);

  const int tid = threadIdx.x;
  const int lane = tid & 63, wave = tid >> 6;
  const int lr = lane & 31, lh = lane >> 5;

  RES_STAMP(10);
  // ---- weights -> LDS, once ----
  {
    const unsigned char* g1 = (const unsigned char*)a.W1;
    const unsigned char* g2 = (const unsigned char*)a.W2c;
    for (int idx = tid; idx < 2 * 384 * 12; idx += (int)blockDim.x) {
      const int which = idx >= 384 * 12;
      const int k2 = which ? idx - 384 * 12 : idx;
      const int row = k2 / 12, k16 = k2 - row * 12;
      const u32x4 v = *(const u32x4*)((which ? g2 : g1) + (int64_t)k2 * 16);
      *(u32x4*)(smem + (which ? MlpResSmem::kW2 : MlpResSmem::kW1) + row * ROW + mlp_res_swz(row, k16) * 16) = v;
    }
    float* sf = reinterpret_cast<float*>(smem + MlpResSmem::kB1);
    for (int i = tid; i < 384 + 96 + 96; i += (int)blockDim.x)
      sf[i] = i < 384 ? a.b1[i] : (i < 480 ? a.b2[i - 384] : a.gamma[i - 480]);
    if (tid == 0) *reinterpret_cast<int*>(smem + MlpResSmem::kCtr) = (int)blockDim.x >> 6;   // slots 0 .. nwaves-1 are taken
    if (LNP) {
      float* sl = reinterpret_cast<float*>(smem + MlpResSmem::kLn);
      for (int i = tid; i < 192; i += (int)blockDim.x) sl[i] = i < 96 ? a.lnp.w[i] : a.lnp.b[i - 96];
    }
  }
  __syncthreads();
  RES_STAMP(11);

  const T* __restrict__ Xp = (const T*)a.X;
  const T* Rp = (const T*)a.resid;
  T* Op = (T*)a.out;

  const int ntiles = (a.M + 31) / 32;
  const int nwaves = (int)blockDim.x >> 6;
  const int stride = (int)gridDim.x * nwaves;
  // lane-constant parts of the fragment addresses: row r = 32*blk + lr has swizzle key (lr >> 2) & 3 (32*blk adds 0 mod 4
  // to r >> 2 ... only when blk*8 is a multiple of 4, which it is)
  const int key = (lr >> 2) & 3;
  const int rowoff = lr * ROW;

  // x_ln fragments (k-step p, lane = token lr / k half lh).  The registers are dead once the last GEMM1 of a tile has
  // issued, so the NEXT tile's rows are fetched there and land under this tile's tail and epilogue.
  u32x4 xf[KP1];
  auto load_x = [&](int tile) {
    const int64_t mm = (int64_t)tile * 32 + lr;
    const int64_t mmc = (GCV_MLP_ABLATE & 8) ? (int64_t)lr : (mm < a.M ? mm : (int64_t)a.M - 1);
#pragma unroll
    for (int p = 0; p < KP1; ++p) xf[p] = *(const u32x4*)(Xp + mmc * C + 16 * p + 8 * lh);
  };
  // Tiles are handed out dynamically inside the workgroup: the two waves of a SIMD do not progress at the same rate
  // (the arbiter serves the older one first: wave 0 finished its static share after 375k cycles, wave 7 after 513k,
  // alone on its SIMD and therefore at half the vector issue rate for the last quarter).  Slot q of this workgroup
  // is tile blockIdx * nwaves + q % nwaves + (q / nwaves) * stride — the same set of tiles as the static walk — and a
  // wave takes its next slot from an LDS counter at the START of a tile, so the next rows can still be prefetched.
  int* const ctr = reinterpret_cast<int*>(smem + MlpResSmem::kCtr);
  auto slot_tile = [&](int q) { return (int)blockIdx.x * nwaves + (q % nwaves) + (q / nwaves) * stride; };
  auto next_slot = [&]() {
    int q = 0;
    if (lane == 0) q = atomicAdd(ctr, 1);
    return __builtin_amdgcn_readfirstlane(q);
  };
  if (slot_tile(wave) < ntiles) load_x(slot_tile(wave));
  int titer = 0;
  for (int tile = slot_tile(wave), tile_next = 0; tile < ntiles; tile = tile_next, ++titer) {
    tile_next = slot_tile(next_slot());
    if (titer == 2) GCV_STAMP(0);
#if GCV_MLP_STAMPS
    if (titer == 2 && blockIdx.x < 64 && threadIdx.x == 0) gcv_mlp_stamps[blockIdx.x * 16 + 8] = __builtin_amdgcn_s_memrealtime();
#endif
    const int64_t m = (int64_t)tile * 32 + lr;
    const int64_t mc = m < a.M ? m : (int64_t)a.M - 1;        // clamp: tail rows compute garbage, store nothing
    const int64_t mld = (GCV_MLP_ABLATE & 8) ? (int64_t)lr : mc;


    // (Peeling the first loop iteration would make this zero the inline constant of the first MFMAs' C operand and save
    // the 48 v_mov_b32 per tile, bit for bit, as xs_mlp_kernel does; here it costs 8 more VGPRs, so it is not done.
    // Starting at b2 instead would save the epilogue's adds too, but changes the order of the fp32 sum and with it
    // the last bit of some outputs.)
    f32x16 acc2[NO];
#pragma unroll
    for (int o = 0; o < NO; ++o)
#pragma unroll
      for (int r = 0; r < 16; ++r) acc2[o][r] = 0.0f;

    // Per-wave software pipeline over the 12 hidden groups of 32.  In steady state one step holds
    //     12 MFMAs :  N += W1[g+1] . x   (N was pre-loaded with b1[g+1] straight from LDS, so the bias add is free)
    //                 acc2 += W2[:, g-1] . h(g-1)
    //     ~175 VALU:  h(g) = GELU(C)  packed to two 16-byte B fragments
    // which are independent of each other, and sched_group_barrier interleaves them 1 MFMA : 15 VALU so the wave never
    // sits out the 32 cycles an MFMA holds the matrix pipe (12 x 32 = 384 of ~1150 cycles per step when the MFMAs are
    // issued back to back).  The LDS reads of the next step (b1 -> accumulator registers, W1 / W2 fragments) are
    // issued at the end of a step, after the MFMAs that used the previous fragments.
    auto frag_off = [&](int k16) { return ((k16 & ~3) | ((k16 & 3) ^ key)) << 4; };
    auto read_w1 = [&](int g, u32x4 (&wf)[KP1]) {
      const unsigned char* base = sW1 + g * 32 * ROW + rowoff;
#pragma unroll
      for (int p = 0; p < KP1; ++p) wf[p] = *(const u32x4*)(base + frag_off(2 * p + lh));
    };
    auto read_w2 = [&](int g, u32x4 (&w2f)[2][NO]) {
      const int ch = g / 3, j = g - 3 * ch;
      const unsigned char* base = sW2 + ch * HC * ROW + rowoff;
#pragma unroll
      for (int s = 0; s < 2; ++s)
#pragma unroll
        for (int o = 0; o < NO; ++o) w2f[s][o] = *(const u32x4*)(base + 32 * o * ROW + frag_off(2 * (2 * j + s) + lh));
    };
    auto read_b1 = [&](int g, f32x16& acc) {               // accumulator := bias of group g (token-on-lane layout;
                                                           // not shared with the xs kernels: see xs_mlp_kernel's step)
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        const f32x4 bv = *(const f32x4*)(sB1 + g * 32 + 8 * q + 4 * lh);
#pragma unroll
        for (int e = 0; e < 4; ++e) acc[4 * q + e] = bv[e];
      }
    };
    auto mfma1 = [&](const u32x4 (&wf)[KP1], f32x16& acc1) {
#pragma unroll
      for (int p = 0; p < KP1; ++p) Mfma<T>::run(wf[p], xf[p], acc1);
    };
    auto mfma2 = [&](const u32x4 (&w2f)[2][NO], const u32x4 (&hf)[2]) {
#pragma unroll
      for (int s = 0; s < 2; ++s)
#pragma unroll
        for (int o = 0; o < NO; ++o) Mfma<T>::run(w2f[s][o], hf[s], acc2[o]);
    };
    auto gelu = [&](const f32x16& acc1, u32x4 (&hf)[2]) {
#pragma unroll
      for (int q0 = 0; q0 < 4; q0 += 2) {
        float hx[8];
#pragma unroll
        for (int c = 0; c < 8; ++c) hx[c] = acc1[4 * q0 + c];
        uint32_t hw[4];
        if (!(GCV_MLP_ABLATE & 1)) gelu_h16_frag<T, 8>(hx, hw);
        else {
          typedef T t2 __attribute__((ext_vector_type(2)));
#pragma unroll
          for (int c = 0; c < 4; ++c) hw[c] = __builtin_bit_cast(uint32_t, (t2){from_f<T>(hx[2 * c]), from_f<T>(hx[2 * c + 1])});
        }
#pragma unroll
        for (int c = 0; c < 4; ++c) hf[q0 >> 1][c] = hw[c];
      }
    };
    // one steady-state step for group g: C holds GEMM1(g)+b1, N holds b1(g+1), hp = h(g-1), wf = W1(g+1), w2f = W2(g-1)
    auto step = [&](int g, f32x16& Cacc, f32x16& Nacc, u32x4 (&hp)[2], u32x4 (&hc)[2], u32x4 (&wf)[KP1], u32x4 (&w2f)[2][NO]) {
      __builtin_amdgcn_sched_barrier(0);
      mfma1(wf, Nacc);
      mfma2(w2f, hp);
      gelu(Cacc, hc);
#pragma unroll
      for (int i = 0; i < 12; ++i) {
        __builtin_amdgcn_sched_group_barrier(0x002, 11, 0);   // 11 VALU
        __builtin_amdgcn_sched_group_barrier(0x008, 1, 0);    // 1 MFMA
      }
      __builtin_amdgcn_sched_barrier(0);
      read_b1(g + 2 < NG ? g + 2 : NG - 1, Cacc);            // C's registers are free: they become the next N
      read_w1(g + 2 < NG ? g + 2 : NG - 1, wf);
      read_w2(g, w2f);
      __builtin_amdgcn_sched_barrier(0);
    };

    f32x16 accA, accB;
    u32x4 wf[KP1], w2f[2][NO], hfA[2], hfB[2];
    read_b1(0, accA);
    read_w1(0, wf);
    mfma1(wf, accA);
    __builtin_amdgcn_sched_barrier(0);
    read_b1(1, accB);
    read_w1(1, wf);
    mfma1(wf, accB);
    __builtin_amdgcn_sched_barrier(0);
    if (titer == 2) GCV_STAMP(1);
    // residual rows: issued a whole tile ahead of the epilogue that adds them (issued in the tail they cost the
    // epilogue ~4k cycles of exposed load latency per tile)
    // (16-byte pieces: lanes 0-31 take channels 16p .. 16p+7 of their row, lanes 32-63 the next eight; the epilogue's
    // permlane32 swap — its own inverse — hands every lane the two 8-byte halves its accumulator layout wants)
    u32x4 rres[NO][2];
#pragma unroll
    for (int o = 0; o < NO; ++o)
#pragma unroll
      for (int pr = 0; pr < 2; ++pr) rres[o][pr] = *(const u32x4*)(Rp + mld * C + 32 * o + 16 * pr + 8 * lh);
    gelu(accA, hfA);                                        // h(0)
    read_b1(2, accA);
    read_w1(2, wf);
    read_w2(0, w2f);
#pragma unroll 1
    for (int g = 1; g < NG - 1; g += 2) {
      if (titer == 2 && g == 1) GCV_STAMP(2);
      step(g, accB, accA, hfA, hfB, wf, w2f);               // odd g : C = B, N = A, h(g-1) in hfA -> h(g) in hfB
      if (titer == 2 && g == 1) GCV_STAMP(3);
      step(g + 1, accA, accB, hfB, hfA, wf, w2f);           // even g: C = A, N = B
      if (titer == 2 && g == 1) GCV_STAMP(4);
    }
    if (titer == 2) GCV_STAMP(5);
    // tail: g = NG-1 sits in accB, h(NG-2) in hfA, w2f = W2(NG-2)
    __builtin_amdgcn_sched_barrier(0);
    if (tile_next < ntiles) load_x(tile_next);
    __builtin_amdgcn_sched_barrier(0);
    mfma2(w2f, hfA);
    gelu(accB, hfB);
    __builtin_amdgcn_sched_barrier(0);
    read_w2(NG - 1, w2f);
    mfma2(w2f, hfB);

    if (titer == 2) GCV_STAMP(7);
    // ---- epilogue: (acc2 + b2) * gamma + resid -> 16-bit, 16-byte pieces ----
    // (LDS offsets through an empty asm: keeps the loop-invariant b2 / gamma LDS reads inside the tile loop, unspilled;
    // offsets rather than pointers, which would come back generic and make the reads flat loads)
    int oB2 = MlpResSmem::kB2, oG = MlpResSmem::kG;
    asm volatile("" : "+s"(oB2), "+s"(oG));
    const float* const sB2t = reinterpret_cast<const float*>(smem + oB2);
    const float* const sGt = reinterpret_cast<const float*>(smem + oG);
    // A row's 16 bytes (o, q) are split over the half-waves (lane lr: channels 8q .. 8q+3, lane lr+32: 8q+4 .. 8q+7).
    // The permlane32 exchange (mlp_parts.h) of a (q, q+1) pair leaves lanes 0-31 with the 16 contiguous bytes of piece q
    // and lanes 32-63 with those of piece q+1: six 16-byte stores per tile instead of twelve 8-byte ones (each store
    // instruction touches 32 rows; the epilogue was 5.6k of a tile's 26k cycles, bound by store issue).
    // LNP: the values go back into the accumulators instead, with their sum and sum of squares.
    // (xs_mlp_kernel's epilogue is this one with 4 lh in the pointers.  Shared __forceinline__ functions for this loop, the
    // patch position and the normalising store were tried: the loop and the store each came out one VGPR lower with the
    // code around them reordered, the patch position reordered the LNP variant; none reproduced the code, so they stay.)
    float s1 = 0.0f, s2 = 0.0f;
#pragma unroll
    for (int o = 0; o < NO; ++o)
#pragma unroll
      for (int q = 0; q < 4; q += 2) {
        vec4<T> rr[2];
        piece_to_halves<T>(rres[o][q >> 1], rr);
        uint2 pk[2];
#pragma unroll
        for (int d = 0; d < 2; ++d) {
          const int n = 32 * o + 8 * (q + d) + 4 * lh;
          const f32x4 bv = *(const f32x4*)(sB2t + n);
          const f32x4 gv = *(const f32x4*)(sGt + n);
          vec4<T> o4;
#pragma unroll
          for (int e = 0; e < 4; ++e) {
            const float v = fmaf(acc2[o][4 * (q + d) + e] + bv[e], gv[e], to_f(rr[d][e]));
            if constexpr (LNP) {
              acc2[o][4 * (q + d) + e] = v;
              s1 += v;
              s2 = fmaf(v, v, s2);
            } else {
              o4[e] = from_f<T>(v);
            }
          }
          if constexpr (!LNP) pk[d] = __builtin_bit_cast(uint2, o4);
        }
        if constexpr (!LNP) {
          const u32x4 w = halves_to_piece(pk);
          const int n16 = 32 * o + 8 * q + 8 * lh;           // lanes 0-31: channels 8q .. 8q+7, lanes 32-63: 8q+8 .. 8q+15
          if (m < a.M && (!(GCV_MLP_ABLATE & 8) || w[0] == 0x12345u)) *(u32x4*)(Op + m * C + n16) = w;
        }
      }
    if constexpr (LNP) {
      // ---- out = LayerNorm2d(resid + gamma * (acc2 + b2)) at the patch position of token m
      float rstd, nmr;
      lnp_stats<C, true>(acc2, s1, s2, a.lnp.eps, rstd, nmr);   // the centred squares under a branch: registers allow it here
      // patch position of this lane's token: segment, image, (y, x) -> patch row and the quarter of its 4C columns
      int sg = 0;
#pragma unroll
      for (int t = 1; t < 4; ++t) sg += (t < a.lnp.nseg && (int)mc >= a.lnp.tok0[t]) ? 1 : 0;
      const int local = (int)mc - a.lnp.tok0[sg];
      const int hw = a.lnp.hw[sg], wd = a.lnp.wd[sg];
      const int img = local / hw, rem = local - img * hw;
      const int py = rem / wd, px = rem - py * wd;
      const int64_t prow = (int64_t)a.lnp.out0[sg] + ((int64_t)img * (hw / wd / 2) + (py >> 1)) * (wd >> 1) + (px >> 1);
      T* const dst = Op + prow * (4 * C) + ((py & 1) * 2 + (px & 1)) * C;
      int oLn = MlpResSmem::kLn;
      asm volatile("" : "+s"(oLn));
      const float* const sLw = reinterpret_cast<const float*>(smem + oLn);
#pragma unroll
      for (int o = 0; o < NO; ++o)
#pragma unroll
        for (int q = 0; q < 4; q += 2) {
          uint2 pk[2];
#pragma unroll
          for (int d = 0; d < 2; ++d) {
            const int n = 32 * o + 8 * (q + d) + 4 * lh;
            const f32x4 wv = *(const f32x4*)(sLw + n);
            const f32x4 cv = *(const f32x4*)(sLw + 96 + n);
            vec4<T> o4;
#pragma unroll
            for (int e = 0; e < 4; ++e) o4[e] = from_f<T>(fmaf(fmaf(acc2[o][4 * (q + d) + e], rstd, nmr), wv[e], cv[e]));
            pk[d] = __builtin_bit_cast(uint2, o4);
          }
          const u32x4 w = halves_to_piece(pk);
          const int n16 = 32 * o + 8 * q + 8 * lh;
          if (m < a.M) *(u32x4*)(dst + n16) = w;
        }
    }
    if (titer == 2) GCV_STAMP(6);
#if GCV_MLP_STAMPS
    if (titer == 2 && blockIdx.x < 64 && threadIdx.x == 0) gcv_mlp_stamps[blockIdx.x * 16 + 9] = __builtin_amdgcn_s_memrealtime();
#endif
  }
  RES_STAMP(12);
}

template <typename T> int launch_fused_mlp_res(const MlpArgs& a, hipStream_t s, int wg_cap = kMlpWgCap);

}  // namespace gcv
