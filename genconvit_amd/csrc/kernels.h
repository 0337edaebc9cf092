// Non-GEMM kernels of the GenConViT path: HBM-bound NHWC kernels with
// fp32 math, 64-lane wave reductions and LDS-staged cross-channel statistics.
//   K3  stem conv4x4s4 + LayerNorm2d            stem_ln_kernel
//   K4  depthwise 7x7 + LayerNorm               dwconv7_ln_kernel
//   K6  LayerNorm2d + 2x2 space-to-depth        ln_patchify_kernel   (conv2x2s2 itself is a GEMM)
//   K7  global-avg-pool + LayerNorm2d           pool_ln_kernel       (fc is a GEMM)
//   K1/K9 first 3->16 conv (Cin=3 is not MFMA-shaped)   conv3_first_kernel
//   K2/K12 last 16->3 ConvTranspose2d           convt2_small_kernel
//   K10/K11 split-K reduce + bias + reparameterise      reparam_kernel, kl_rows_kernel
//   K8  500->2 head tail                        head_tail_kernel
//   K13/K14 bilinear 112->224 (+ per-frame MSE) resize_mse_kernel
//   K15 sigmoid -> mean over rows               vote_kernel
#pragma once
#include "common.h"

namespace gcv {

// ------------------------------------------------------------------ launch wrappers (defined in kernels_impl.h)
template <typename T> int launch_stem_ln(const T* x, int64_t sb, int64_t sc, int64_t sy, int64_t sx, const float* wp,
                                         const float* bias, const float* lnw, const float* lnb, T* out, int nimg,
                                         int Ho, int Wo, float eps, hipStream_t s, int C = 96);
// depthwise 7x7 + LayerNorm (dwconv_impl.h): the kernel that runs a launch of nimg H x W x C images and its grid, planned
// in one place (dw_select); dw_plan returns the plan, or the launcher's error, without a HIP call.  The tile kinds are
// compiled in the kern_*.hip translation units and launched from the plan by launch_dw_tile (kernels_impl.h)
enum class DwKind { Tile, Tiny, TinyPair, Roll, Mfma, Pair };   // in this order: the `kind` of gcv_dw_plan
struct DwPlan {
  DwKind kind = DwKind::Tile;
  int C = 0, n = 0;                   // template shape: C, and NS = W / 7 (Roll, Mfma, Pair) or S = H = W (Tiny, TinyPair)
  int band_rows = 0;                  // Roll, Mfma, Pair: output rows per workgroup
  int grid = 0, block = 0, lds = 0;   // workgroups, threads per workgroup, dynamic LDS bytes
};
template <typename T> int dw_plan(DwPlan& p, int nimg, int H, int W, int C, bool aligned);   // aligned: x, y 16-byte
template <typename T> int launch_dwconv7_ln(const T* x, const float* wdw, const float* bdw, const float* lnw,
                                            const float* lnb, T* y, int nimg, int H, int W, int C, float eps,
                                            hipStream_t s, int plan_nimg = 0);   // plan_nimg: dw_select, test entries only
// two image groups of one C (group 0 the wider map) behind one another in ONE grid where dw_select's kernels for them are
// a pair dwconv_impl.h has a merged kernel for (dw_two_merged says so without a HIP call), in two launches otherwise; each
// group's kernel, bands and workgroups are those of launch_dwconv7_ln on it alone, and so is every output bit
template <typename T> bool dw_two_merged(int nimg0, int H0, int W0, int nimg1, int H1, int W1, int C, bool aligned);
template <typename T> int launch_dwconv7_ln2(const T* x0, T* y0, int nimg0, int H0, int W0, const T* x1, T* y1, int nimg1,
                                             int H1, int W1, const float* wdw, const float* bdw, const float* lnw,
                                             const float* lnb, int C, float eps, hipStream_t s, int plan_nimg0 = 0,
                                             int plan_nimg1 = 0);
template <typename T> int launch_dw_tile(const DwPlan& p, const T* x, const float* wdw, const float* bdw, const float* lnw,
                                         const float* lnb, T* y, int nimg, int H, int W, float eps, hipStream_t s);
// launches kernel with p's grid, block and dynamic LDS (raising the kernel's limit first where p needs more than 64 KiB)
template <class K, class... A> int dw_launch(const DwPlan& p, K kernel, hipStream_t s, A... args) {
  if (p.lds > 64 * 1024) GCV_ENSURE_LDS(kernel, p.lds);
  hipLaunchKernelGGL(kernel, dim3(p.grid), dim3(p.block), p.lds, s, args...);
  GCV_CHECK_HIP(hipGetLastError());
  return 0;
}
template <typename T> int launch_ln_patchify(const T* x, const float* w, const float* b, T* out, int nimg, int H,
                                             int W, int C, float eps, hipStream_t s);
template <typename T> int launch_layernorm_rows(const T* x, const float* w, const float* b, T* out, int64_t rows,
                                                int C, float eps, hipStream_t s);
// seg_n > 0: image b of the launch -> output row (b % seg_n) * row_stride + row0 + b / seg_n (see pool_ln_kernel)
template <typename T> int launch_pool_ln(const T* x, const float* w, const float* b, T* out, int nimg, int HW, int C,
                                         float eps, hipStream_t s, int seg_n = 0, int row_stride = 1, int row0 = 0);
template <typename T> int launch_conv3_first(const T* x, int64_t sb, int64_t sc, int64_t sy, int64_t sx,
                                             const float* wp, const float* bias, T* out, int nimg, int H, int W,
                                             bool pool, int act, hipStream_t s);
template <typename T> int launch_convt2_small(const T* x, const float* wp, const float* bias, T* out, int nimg, int H,
                                              int W, int act, hipStream_t s);
template <typename T> int launch_reparam(const float* partial, int splitk, const float* bias, const float* eps,
                                         float* mu_out, T* z_nhwc, int B, int N, hipStream_t s);
template <typename T> int launch_head_tail(const T* h, const float* w, const float* bias, float* logits, int B, int K,
                                           hipStream_t s);
// the same with the hidden layer's split-K partials (S, B, K) fp32 reduced on the way in: h = act(sum + b1)
template <typename T> int launch_head_tail_splitk(const float* partial, int S, const float* b1, int act, const float* w,
                                                  const float* bias, float* logits, int B, int K, hipStream_t s);
template <typename T> int launch_resize_mse(const T* xhat, const T* img, T* recon, float* msepart, float* mse, int B,
                                            hipStream_t s);
template <typename T> int launch_swin_window_attn(const T* qkv, const float* rpb, T* out, int nimg, int H, int W, int C,
                                                  int nH, int shift, hipStream_t s);
template <typename T> int launch_patch_merge_ln(const T* x, const float* w, const float* b, T* out, int nimg, int H,
                                                int W, int C, float eps, hipStream_t s);
template <typename T> int launch_mean_tokens(const T* x, T* out, int nimg, int L, int C, hipStream_t s);
template <typename T> int launch_preprocess(const unsigned char* u8, T* out, int n, int H, int W, hipStream_t s);
// N4 (face.hip): crop + cv2.INTER_AREA resize of n face boxes, uint8 RGB
int launch_face_crop_resize(const unsigned char* frames, int nframes, int H, int W, const int* boxes5, int n,
                            unsigned char* out, int S, hipStream_t s);
// the same crop pixels, normalised like launch_preprocess and written as NCHW in T: one launch, no uint8 image in between
template <typename T> int launch_face_crop_preprocess(const unsigned char* frames, int nframes, int H, int W,
                                                      const int* boxes5, int n, T* out, int S, hipStream_t s);
// overlay.hip: evidence maps drawn over their face boxes as a colour heat overlay, uint8 RGB frames in and out
int launch_cam_overlay(const unsigned char* frames, int nframes, int H, int W, const int* boxes5, int n, const float* maps,
                       int mh, int mw, const unsigned char* lut768, float alpha, int weighted, unsigned char* out,
                       hipStream_t s);
// annotate.hip: a scan's marks (outline, number tab) and its timeline strip drawn onto the frames, uint8 RGB in and out
int launch_scan_annotate(const unsigned char* frames, int nframes, int H, int W, const int* frame_no, const int* marks8,
                         int n, const unsigned* timeline, int lanes, int T, int strip, unsigned char* out, hipStream_t s);
// yuv.hip: decoder-native YUV 4:2:0 frames (layout 0 = i420, 1 = nv12; matrix 0 = bt601, 1 = bt709) to the uint8 RGB slab,
// and an RGB slab back to YUV 4:2:0
int launch_yuv420_to_rgb(const unsigned char* yuv, int nframes, int H, int W, int layout, int matrix, int full_range,
                         unsigned char* rgb, hipStream_t s);
int launch_rgb_to_yuv420(const unsigned char* rgb, int nframes, int H, int W, int layout, int matrix, int full_range,
                         unsigned char* yuv, hipStream_t s);
// follow.hip: block matching of a face between two detector frames, n jobs of 17 ints -> n rows (oy, ox, cost, cost0)
int launch_track_match(const unsigned char* frames, int nframes, int H, int W, const int* jobs17, int n, int grid,
                       int radius, int* out4, hipStream_t s);
// the same search walked along a chain of frames, each step around the box of the step before: n jobs of 11 ints ->
// n x max_steps rows (oy, ox, cost, cost0)
int launch_track_chain(const unsigned char* frames, int nframes, int H, int W, const int* jobs11, int n, int max_steps,
                       int grid, int radius, int* out4, hipStream_t s);
// cuts.hip: 64-bin luma histograms of the regions x regions parts of every frame, and their L1 distance between
// consecutive frames
int launch_frame_hist(const unsigned char* frames, int nframes, int H, int W, int regions, uint32_t* hist, hipStream_t s);
int launch_hist_diff(const uint32_t* hist, int nframes, int regions, uint32_t* dist, hipStream_t s);
int launch_hist_diff_lag(const uint32_t* hist, int nframes, int regions, int lag, uint32_t* dist, hipStream_t s);
int launch_frame_cells(const unsigned char* frames, int nframes, int H, int W, int grid, uint32_t* cells, hipStream_t s);
int launch_blend_fit(const uint32_t* cells, int nframes, int grid, int lag, int64_t* fit, hipStream_t s);
// quality.hip: sharpness, gradient and exposure sums of n face boxes on a grid x grid lattice of mean-luma cells ->
// n rows (G, S1, S2, L2, GX, GY, dark, bright)
int launch_face_quality(const unsigned char* frames, int nframes, int H, int W, const int* boxes5, int n, int grid,
                        int64_t* out8, hipStream_t s);
// persons.hip: n face boxes -> n appearance signatures of 384 bytes, and the (T, T) minimum L1 distance between the rows
// of every two tracks
int launch_face_signature(const unsigned char* frames, int nframes, int H, int W, const int* boxes5, int n,
                          unsigned char* out384, hipStream_t s);
int launch_sig_link(const unsigned char* sig, const int* owner, int n, int T, uint32_t* out, hipStream_t s);
int launch_kl(const float* partial, int splitk, const float* bias, const float* mu, float* rowsum, float* kl, int B,
              int N, hipStream_t s);
int launch_vote(const float* logits, int rows, float* mean2, hipStream_t s);
int launch_vote_segments(const float* logits, int B, int nets, const int* off, int nvid, float* mean2, hipStream_t s);
int launch_vote_windows(const float* logits, int B, int nets, const int* ranges2, int n_ranges, float* frame_p,
                        float* mean2, hipStream_t s);

}  // namespace gcv
