// Grad-CAM of the networks' real / fake logit at the last ConvNeXt stage (gcv_*_explain, include/genconvit_hip.h).
//
// The backbone ends in global-avg-pool -> LayerNorm2d -> fc, so d logit / d A_c(h, w) is the same at every position of the
// stage-3 map A: the explain path is the backward of the heads alone, then one dot product per stage-3 token.
//   head_bwd_kernel   target logit -> fc2^T -> act'(hidden) -> fc^T (500 -> 2000) -> act'(backbone logits): d feat (B, 2000)
//   bb_bwd_kernel     backbone fc^T (1000 -> 768) per frame and pass: d pooled-LayerNorm output (2B, 768)
//   cam_kernel        LayerNorm2d backward on the pooled row (mean / rstd recomputed from the stage-3 tokens) -> g (768),
//                     CAM(h, w) = ReLU(sum_c g_c A_c(h, w)), optional bilinear upsample to 224 x 224
// All gradient math is fp32; activations and weights are read in the storage dtype.
#pragma once
#include "common.h"

namespace gcv {

struct HeadBwdArgs {
  const float* partial;   // (S, B, 500) fp32 split-K partials of the head's fc (the forward's, kept alive)
  int S;
  const float* b1;        // fc bias (500)
  const float* fc2_w;     // (2, 500) fp32
  const float* logits;    // (B, 2) fp32: the argmax when target is null
  const int* target;      // (B) device ints, nullable; a value != 0 selects class 1
  const void* fc_w;       // (500, 2000) T
  const void* bb_pre;     // (B, 2000) T: backbone logits before the activation
  float* dfeat;           // (B, 2000) fp32 out: d logit / d backbone logits
  int B, act;
};
struct CamArgs {
  const void* A[2];       // stage-3 tokens of pass p: image b at A[p] + b * hw[p] * C, (hw, C) in T (C: launch_cam's)
  int hw[2], side[2];     // side * side = hw
  int cam_off[2];         // map of (b, p) at cam + b * cam_ld + cam_off[p]
  int npass, cam_ld, up_pass;
  const float* lnw;       // head.norm.weight (C)
  const float* dpool;     // (B, npass, C) fp32: d logit / d LayerNorm output
  float* cam;
  float* cam224;          // nullable: (B, 224, 224) fp32 upsample of pass up_pass's map
  float eps;
  int B;
};

template <typename T> int launch_head_bwd(const HeadBwdArgs& a, hipStream_t s);
// d pooled row (rows, C) = dfeat rows (rows, 1000) . W, W = head.fc.weight (1000, C) in T; C = 768 (ConvNeXt-T) or 1536 (-L)
template <typename T> int launch_bb_bwd(const float* dfeat, const void* W, float* dpool, int rows, int C, hipStream_t s);
template <typename T> int launch_cam(const CamArgs& a, int C, hipStream_t s);

}  // namespace gcv
