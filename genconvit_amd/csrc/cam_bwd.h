// Grad-CAM one stage earlier (gcv_*_explain_at, layer = 2): the data-gradient backward of ConvNeXt stage 3 and of the
// stage 2 -> 3 down-sampling, from d logit / d (pooled LayerNorm output) (cam.h: head_bwd_kernel -> bb_bwd_kernel) down to
// d logit / d A2, the stage-2 output.  The schedule is NetImpl::explain_tail_s2 (net_impl.h).
//
//   pool_ln_bwd_kernel    pooled LayerNorm2d backward + average-pool backward: the same row g / hw for every token of an image
//   scale_rows_kernel     fp32 gradient rows [* layer scale gamma] -> the storage dtype, each row times a power of two that
//                         brings its largest magnitude into [0.5, 1) (exact; rows of dY . W are independent), so that a
//                         16-bit MFMA operand never sits in fp16 subnormals; the inverse factor is kept per row
//   gelu_bwd_kernel       dh * GELU'(pre) at the recomputed hidden pre-activation (exact erf), unscaled, re-scaled per row
//   dw_ln_bwd_kernel      raw depthwise 7 x 7 output of a token with its LayerNorm statistics (the forward stores only the
//                         LayerNorm output), then the LayerNorm backward over the row; maps of at most 7 x 7
//   dw_dgrad_res_*        depthwise 7 x 7 data gradient (flipped-tap correlation, zero padding, per image) + residual add;
//                         for the 7 x 7 and 3 x 3 maps one thread keeps a channel's map and taps in registers
//   down_ln_bwd_kernel    depth-to-space of the patch gradient back to the stage-2 grid (an odd last row / column gets zero)
//                         + LayerNorm2d backward over C2 with the stored stage-2 tokens
//   cam2_kernel           alpha = spatial mean of d A2 per image, CAM = ReLU(sum_c alpha_c A2_c), optional 224 x 224 upsample
// The contractions between them (dz . W2, dpre . W1, dx . W_down and the pre-activation recompute) run on the matrix pipe
// through launch_gemm (gemm.h) with fp32 output (EPI_SPLITK, one split).  Gradients in memory are fp32.
#pragma once
#include "common.h"

namespace gcv {

// d pooled-LayerNorm output (B, npass, C) -> dA (rows of pass p, image b at (tok0[p] + b * hw[p]), C) fp32
struct PoolLnBwdArgs {
  const void* A[2];       // stage-3 tokens of pass p (hw[p], C) per image, in T
  int hw[2], tok0[2];
  int npass, B;
  const float* lnw;       // head.norm.weight (C)
  const float* dpool;     // (B, npass, C) fp32
  float* dA;              // (M, C) fp32
  float eps;
};
template <typename T> int launch_pool_ln_bwd(const PoolLnBwdArgs& a, int C, hipStream_t s);

// out (M, C) T = g (M, C) * gamma (nullable) * 2^e(row); inv[row] = 2^-e(row).  C = 768 / 1536.
template <typename T> int launch_scale_rows(const float* g, const float* gamma, T* out, float* inv, int M, int C, hipStream_t s);

// pre (M, C4) T in place: pre <- dh * inv_in[row] * GELU'(pre) * 2^e(row); inv_out[row] = 2^-e(row)
template <typename T> int launch_gelu_bwd(const float* dh, const float* inv_in, T* pre, float* inv_out, int M, int C4, hipStream_t s);

// one pass of nimg images with side x side maps (side <= 7): x the block's input tokens (T), dxln (rows, C) fp32 the scaled
// gradient of the LayerNorm output with its per-row inverse scale, ddw (rows, C) fp32 out: gradient of the raw depthwise output
struct DwLnBwdArgs {
  const void* x;
  const float *dw_w, *dw_b, *ln_w;   // taps [49][C], bias (C), LayerNorm weight (C)
  const float *dxln, *inv;
  float* ddw;
  int nimg, side;
  float eps;
};
template <typename T> int launch_dw_ln_bwd(const DwLnBwdArgs& a, int C, hipStream_t s);

// g (rows, C) fp32 in place: g += depthwise data gradient of ddw (rows, C); nimg images of side x side tokens
int launch_dw_dgrad_res(const float* ddw, const float* dw_w, float* g, int nimg, int side, int C, hipStream_t s);

// one pass: stage-2 tokens x (nimg, side2, side2, C2) in T; dP (nimg * (side2 / 2)^2, 4 C2) fp32 scaled patch gradient,
// columns (ky, kx, ci), with its per-row inverse scale; dA2 (nimg * side2^2, C2) fp32 out
struct DownLnBwdArgs {
  const void* x;
  const float* ln_w;
  const float *dP, *inv;
  float* dA2;
  int nimg, side2;
  float eps;
};
template <typename T> int launch_down_ln_bwd(const DownLnBwdArgs& a, int C2, hipStream_t s);

struct Cam2Args {
  const void* A[2];       // stage-2 tokens of pass p, in T
  const float* dA2[2];    // their gradient, fp32
  int side[2];            // map side of pass p (at most 14)
  int cam_off[2];         // map of (b, p) at cam + b * cam_ld + cam_off[p]
  int npass, cam_ld, up_pass, B;
  float* cam;
  float* cam224;          // nullable: (B, 224, 224) fp32 upsample of pass up_pass's map
  float* alpha;           // (npass, B, C2) fp32 out
};
template <typename T> int launch_cam2(const Cam2Args& a, int C2, hipStream_t s);

}  // namespace gcv
