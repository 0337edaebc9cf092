/* genconvit_hip.h — C ABI of libgenconvit_hip.so (MI355X / gfx950 only).
 *
 * Drop-in boundary for the GenConViT `ed` + `vae` inference forward.  The reference
 * (ctxnn/GenConViT, pure PyTorch) has no FFI layer; each entry point below replaces the
 * Python/ATen call it cites (paths relative to the reference root).  A maintainer binds
 * these with ctypes/cffi exactly as genconvit_amd/_lib.py does.
 *
 * Conventions
 *   - all pointers are device pointers (e.g. torch.Tensor.data_ptr()) unless stated otherwise
 *   - `gcv_stream` is a hipStream_t (torch.cuda.current_stream().cuda_stream); work is enqueued,
 *     never synchronised, by the forward calls
 *   - return value 0 = ok; non-zero = error, text via gcv_last_error() (thread-local)
 *   - a handle owns its packed weights + workspace; not thread-safe; one handle per stream
 *   - the handle-based calls (gcv_*_forward, gcv_load_*) make the handle's device current for their launches and
 *     restore the caller's device before returning; the handle-less calls (gcv_vote*, gcv_preprocess, gcv_k_*)
 *     launch on `stream` as given: the device that owns that stream must be the current one
 *   - frames: (B,3,224,224) NCHW contiguous in the handle's storage dtype, already normalised like
 *     model/pred_func.py:95-108 (preprocess_frame); logits are always fp32 (B,2)
 */
#ifndef GENCONVIT_HIP_H
#define GENCONVIT_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#if defined(GCV_BUILD)
#pragma GCC visibility push(default)
#endif

typedef struct gcv_handle gcv_handle;
typedef void* gcv_stream;

enum { GCV_F32 = 0, GCV_BF16 = 1, GCV_F16 = 2 };               /* storage dtype of a handle      */
enum { GCV_CONVNEXT_TINY = 0, GCV_CONVNEXT_LARGE = 1 };        /* ConvNeXt backbone of a handle  */
enum { GCV_LARGE_MAX_BATCH = 256 };                            /* max_batch cap of a Large handle */
enum { GCV_ACT_NONE = 0, GCV_ACT_RELU = 1, GCV_ACT_GELU = 2, GCV_ACT_LEAKY = 3 };

/* One named fp32 tensor of a reference state_dict (key names as in weight/{ed,vae}.pth,
 * SURVEY.md Appendix A.3).  `data` may be host or device memory. */
typedef struct {
  const char* name;
  const void* data;     /* fp32, contiguous */
  int64_t numel;
  int on_device;
} gcv_tensor_desc;

const char* gcv_last_error(void);

/* Handle lifetime.  Replaces GenConViT.__init__'s module construction + .to(device)/.half()
 * (model/genconvit.py:9-64, model/pred_func.py:50-62).  `max_batch` sizes the workspace arena. */
int  gcv_create(gcv_handle** h, int device, int dtype, int max_batch);
/* The same with the ConvNeXt backbone of both networks chosen: GCV_CONVNEXT_TINY (what gcv_create builds; timm
 * convnext_tiny, model/config.yaml:2) or GCV_CONVNEXT_LARGE (timm convnext_large: dims 192/384/768/1536, depths
 * 3/3/27/3), the config that prediction.py --s large writes (prediction.py:314-318, prediction_v2.py:421-423).  The
 * checkpoint keys are the same with the wider shapes and stages.2.blocks.0..26.  A Large handle takes max_batch
 * <= GCV_LARGE_MAX_BATCH (256): the ED network's stage-0 MLP hidden tensor at 512 frames passes 32-bit GEMM indexing.
 * gcv_genconvit_forward / _explain refuse an ED and a VAE handle of different architectures. */
int  gcv_create_arch(gcv_handle** h, int device, int dtype, int max_batch, int arch);
/* the handle's GCV_CONVNEXT_* architecture (-1 for a null handle) */
int  gcv_handle_arch(const gcv_handle* h);
void gcv_destroy(gcv_handle* h);
size_t gcv_workspace_bytes(const gcv_handle* h);

/* Weight loading: replaces load_state_dict of GenConViTED / GenConViTVAE
 * (model/genconvit.py:16-21,30-35,47-56).  Tensors are re-packed once (conv weights to GEMM
 * order, BatchNorm folded, mu/var columns permuted to NHWC, cast to the handle dtype).
 * Keys that never run in forward (embedder.*, *.patch_embed.*, encoder.fc1/fc2, fc3,
 * num_batches_tracked) are ignored; a missing on-path key is an error. */
int gcv_load_ed (gcv_handle* h, const gcv_tensor_desc* w, int n);
int gcv_load_vae(gcv_handle* h, const gcv_tensor_desc* w, int n);
/* Swin-T embedder weights (timm swin_tiny_patch4_window7_224 keys under `prefix`, e.g. "embedder.");
 * constructed-but-never-executed in the reference forward (model/genconvit_ed.py:69-70). */
int gcv_load_swin(gcv_handle* h, const gcv_tensor_desc* w, int n, const char* prefix);

/* GenConViTED.forward (model/genconvit_ed.py:77-88): logits[b] = fc2(gelu(fc(gelu(cat(
 * backbone(decoder(encoder(x))), backbone(x)))))). */
int gcv_ed_forward(gcv_handle* h, const void* x_nchw, int batch, float* logits, gcv_stream stream);

/* GenConViTVAE.forward (model/genconvit_vae.py:107-116) with the encoder's single
 * torch.randn_like draw (model/genconvit_vae.py:46) made an explicit fp32 input `eps` (B,12544).
 *   recon224 : nullable, (B,3,224,224) in the handle dtype = transforms.Resize((224,224))(x_hat) (:116)
 *   mse      : nullable, (B) fp32 per-frame mean((recon224 - x)^2); its mean is the reference's
 *              nn.MSELoss()(recons, images) (train/train_vae.py:24,76)
 *   kl       : nullable, (1) fp32 = Encoder.kl (model/genconvit_vae.py:58)
 * backbone(x) (:111) depends on nothing but the input: called on its own, gcv_vae_forward enqueues it on a side stream
 * owned by the handle, forked from `stream` at the call and joined back into it by an event before the head, while the
 * encoder / decoder chain and backbone(x_hat) run on `stream` itself; inside gcv_genconvit_forward everything of the VAE
 * stays on one stream.  GCV_VAE_SPLIT=0 / 1 (read when the handle is created) forces the merged / the split schedule.
 * Either way nothing changes for the caller: all work is ordered after what `stream` held at the call and before what
 * it is given next; no synchronisation. */
int gcv_vae_forward(gcv_handle* h, const void* x_nchw, const float* eps, int batch, float* logits,
                    void* recon224, float* mse, float* kl, gcv_stream stream);

/* GenConViT.forward for net = 'genconvit' (model/genconvit.py:66-75): logits_2Bx2 = cat((ed(x), vae(x)[0]), dim=0),
 * rows 0..B-1 = ED logits of frames 0..B-1, rows B..2B-1 = VAE logits.  The two networks are independent until the
 * concat: they run on two internal streams forked from `stream` and joined back into it with events, so a C caller
 * gets the overlapped step (one network's small-grid kernels fill the other's tails) without managing streams.
 * `h_ed` / `h_vae`: two handles of one device and dtype with gcv_load_ed / gcv_load_vae done (each owns its own
 * workspace).  eps as in gcv_vae_forward. */
int gcv_genconvit_forward(gcv_handle* h_ed, gcv_handle* h_vae, const void* x_nchw, const float* eps, int batch,
                          float* logits_2Bx2, gcv_stream stream);

/* ---- explain: Grad-CAM evidence maps of each frame's real / fake decision (new capability) ----
 * Each entry runs the corresponding forward above — the same launches, so `logits` are bit-identical to the forward's on
 * the same input (and eps) — and then, on the same stream(s), the backward of the network's head from the target logit
 * to the last ConvNeXt stage: fc2^T, the activation mask (GELU' for ED, ReLU' for the VAE, at the hidden layer and at the
 * backbone logits, using the forward's pre-activations), fc^T (500 -> 2000), the backbone fc^T (1000 -> 768) and the
 * pooled LayerNorm2d's backward.  Average pooling makes d logit / d A_c(h, w) the same vector g (768, fp32) at every
 * position of the stage-3 map A of a pass, so the Grad-CAM weights are g itself and
 *   CAM(h, w) = ReLU(sum_c g_c A_c(h, w))       (fp32, not normalised: callers choose their own scaling)
 * over the stored stage-3 tokens (tap <net>.bb.s3.b2).  The CAM of the reconstruction passes stops at the backbone: it is
 * the map over the reconstructed image, not propagated through the encoder / decoder.
 *   target   nullable (B) int32 device array: class 0 or 1 per frame (a non-zero value means 1); null = the argmax of each
 *            frame's logits (ties -> class 0)
 *   cam_raw  fp32, not null.  ED : [B][2][7][7] — pass 0 = backbone(reconstruction), pass 1 = backbone(x) (the reference's
 *                                  x1, x2 order, model/genconvit_ed.py:82-83)
 *                             VAE: [B][7*7 + 3*3] — backbone(x) at 224 px, then backbone(x_hat) at 112 px
 *   cam224   nullable fp32 (B, 224, 224): F.interpolate(map of backbone(x), size=(224, 224), mode='bilinear',
 *            align_corners=False)
 * The workspace arena created with the handle holds the saved tensors at every batch up to max_batch: no allocation, copy
 * or synchronisation happens inside a call. */
int gcv_ed_explain(gcv_handle* h, const void* x_nchw, int batch, const int* target, float* logits, float* cam_raw,
                   float* cam224, gcv_stream stream);
int gcv_vae_explain(gcv_handle* h, const void* x_nchw, const float* eps, int batch, const int* target, float* logits,
                    float* cam_raw, float* cam224, gcv_stream stream);
/* Both networks as in gcv_genconvit_forward (two internal streams, the same schedule), with their maps in the (2B) row
 * order of the logits: cam_raw = ED block (B x 98 floats, layout above) followed by the VAE block (B x 58 floats);
 * cam224 (2B, 224, 224): rows 0..B-1 the ED maps of x, rows B..2B-1 the VAE's.  `target` (B) applies to both networks;
 * null = each network's own argmax. */
int gcv_genconvit_explain(gcv_handle* h_ed, gcv_handle* h_vae, const void* x_nchw, const float* eps, int batch,
                          const int* target, float* logits_2Bx2, float* cam_raw, float* cam224, gcv_stream stream);

/* ---- explain at a chosen ConvNeXt stage ----
 * The entries above with one more argument, `layer`: the stage whose output the maps are taken at.
 *   layer = 3  exactly gcv_*_explain: the same launches, outputs and layouts.
 *   layer = 2  Grad-CAM at the output of stage 2, the residual stream after the stage's last block (tap <net>.bb.s2.b8 on
 *              ConvNeXt-T, <net>.bb.s2.b26 on -L): 14 x 14 cells of 16 pixels over a 224-pixel crop (7 x 7 for the VAE's
 *              112-pixel pass).  The gradient is no longer constant over the map, so the call continues the backward above
 *              through the pooled LayerNorm2d and the average pool, stage 3's three blocks (layer scale, fc2^T, exact-erf
 *              GELU' at the recomputed hidden pre-activation, fc1^T, LayerNorm backward at the recomputed depthwise output,
 *              the depthwise 7 x 7 data gradient, the residual) and the stage 2 -> 3 down-sampling (conv^T as a GEMM,
 *              depth-to-space, LayerNorm2d backward), all gradient math in fp32, and then
 *                alpha_c   = mean over (h, w) of d logit_target / d A2_c(h, w)
 *                CAM(h, w) = ReLU(sum_c alpha_c A2_c(h, w))        (fp32, not normalised)
 *              cam_raw  ED : [B][2][14][14] (pass order as above)       VAE: [B][14*14 + 7*7]
 *                       ensemble: the ED block (B x 392 floats) followed by the VAE block (B x 245 floats)
 *              cam224   as above, from the 14 x 14 map of backbone(x)
 *              An odd last row / column of a stage-2 map (the 7 x 7 one) takes no part in the down-sampling and has zero
 *              gradient.  In this mode the forward keeps the stage-2 output and the inputs of stage 3's blocks instead of
 *              overwriting them (same kernels, same operands: the logits stay bit-identical to the plain forward's).
 * Any other `layer` is an error (gcv_last_error()).  target, eps, streams, chunking rules and "no allocation, copy or
 * synchronisation inside a call" are those of gcv_*_explain; the handle's arena is sized for either layer at max_batch. */
int gcv_ed_explain_at(gcv_handle* h, const void* x_nchw, int batch, const int* target, int layer, float* logits,
                      float* cam_raw, float* cam224, gcv_stream stream);
int gcv_vae_explain_at(gcv_handle* h, const void* x_nchw, const float* eps, int batch, const int* target, int layer,
                       float* logits, float* cam_raw, float* cam224, gcv_stream stream);
int gcv_genconvit_explain_at(gcv_handle* h_ed, gcv_handle* h_vae, const void* x_nchw, const float* eps, int batch,
                             const int* target, int layer, float* logits_2Bx2, float* cam_raw, float* cam224,
                             gcv_stream stream);

/* timm convnext_tiny forward alone (call sites model/genconvit_ed.py:82-83,
 * model/genconvit_vae.py:111-112): which = 0 the ED backbone, 1 the VAE backbone;
 * x (B,3,res,res) -> logits1000 (B,1000) in the handle dtype.
 * res: a multiple of 4 in [32, 224].  A ConvNeXt-L handle (GCV_CONVNEXT_LARGE) takes [32, 156] and 224 only: at 160 ... 220
 * the last stage's map is 5 or 6 pixels wide, for which there is no C = 1536 depthwise kernel.  Any other res is refused
 * (gcv_last_error() names the range) before anything is launched; a refused or failed call leaves the handle's workspace
 * as it found it. */
int gcv_convnext_forward(gcv_handle* h, int which, const void* x_nchw, int batch, int res,
                         void* logits1000, gcv_stream stream);

/* timm swin_tiny_patch4_window7_224 forward (only executed by HybridEmbed.__init__,
 * model/model_embedder.py:22): x (B,3,224,224) -> (B,1000) in the handle dtype. */
int gcv_swin_forward(gcv_handle* h, const void* x_nchw, int batch, void* logits1000, gcv_stream stream);

/* preprocess_frame (model/pred_func.py:95-108 + the "vid" Normalize of dataset/loader.py:63-65,77) on the device:
 * uint8 NHWC face crops (n,H,W,3) -> ((x/255) - mean) / std as NCHW in `dtype` (row N1 of SURVEY.md §8f). */
int gcv_preprocess(int dtype, const void* frames_u8_nhwc, void* out_nchw, int n, int H, int W, gcv_stream s);

/* Row N4: the crop + resize of face_rec (model/pred_func.py:79-85),
 *   cv2.resize(frame[top:bottom, left:right], (224, 224), interpolation=cv2.INTER_AREA),
 * for n faces in one launch.  frames: (nframes,H,W,3) uint8 RGB on the device; boxes5: int32 device array of n rows
 * (frame index, top, right, bottom, left) — face_recognition's (top, right, bottom, left) order behind the index of the
 * frame the face was found in; out: (n,size,size,3) uint8.  The reference's RGB<->BGR swaps around the resize cancel.
 * A row outside its frame produces zeros (and reads nothing).  Face DETECTION (dlib) and video decode (decord) stay
 * third-party CPU code on the caller's side. */
int gcv_face_crop_resize(const void* frames_u8_nhwc, int nframes, int H, int W, const int* boxes5, int n,
                         void* out_u8_nhwc, int size, gcv_stream s);

/* gcv_face_crop_resize and gcv_preprocess in one launch: the same frames and boxes straight to the network's input,
 * out (n,3,size,size) NCHW in `dtype` (GCV_F32, GCV_BF16 or GCV_F16), no uint8 image in between.  With u8 exactly the byte
 * gcv_face_crop_resize writes for that pixel and channel,
 *   out[b][c][dy][dx] = (T)(((float)u8 / 255.0f - mean_c) / std_c)         (each operation rounded to fp32 on its own),
 * so the result is bit-equal to gcv_preprocess(gcv_face_crop_resize(...)) for all three dtypes.  A row outside its frame
 * writes the value of u8 = 0 (and reads nothing); n == 0 launches nothing.  The call allocates, copies and synchronises
 * nothing. */
int gcv_face_crop_preprocess(int dtype, const void* frames_u8_nhwc, int nframes, int H, int W, const int* boxes5, int n,
                             void* out_nchw, int size, gcv_stream s);

/* The way back of gcv_face_crop_resize: draw each face's evidence map (gcv_*_explain) over its box of the source frame
 * as a colour heat overlay, n boxes in one launch, one read and one write of the frames.
 *   frames  (nframes,H,W,3) uint8 RGB on the device            out  the same shape; out == frames (in place) is allowed
 *   boxes5  int32 device array of n rows (frame, top, right, bottom, left), as for gcv_face_crop_resize
 *   maps    (n,mh,mw) fp32 on the device, one per box, 1 <= mh, mw <= 224; values are taken as [0, 1] (clamped)
 *   lut768  256 x RGB uint8 on the device: the colour of map value k / 255
 *   alpha   blend weight in [0, 1]; weighted != 0 scales it by the map value, so cold regions of a face stay untouched
 * out is a copy of frames in which every pixel inside a box is blended with the colour of that box's map at that
 * position.  Boxes are applied in row order: a later box draws over what an earlier one left, deterministically for
 * overlapping and nested boxes (every pixel is read and written by one thread).  n == 0 copies the frames; a row outside
 * its frame draws nothing.  No allocation, copy or synchronisation inside the call.
 * Arithmetic (fixed, so that a CPU restatement is bit-equal: tests/overlayutil.py).  For row y of a box of height
 * h = bottom - top, j = y - top (columns alike with w, mw, lx):
 *   num = max((2j + 1) mh - h, 0);  i0 = num / 2h;  i1 = min(i0 + 1, mh - 1);  ly = float(num - i0 2h) / float(2h)
 *   v   = (M[i0,j0] (1 - lx) + M[i0,j1] lx) (1 - ly) + (M[i1,j0] (1 - lx) + M[i1,j1] lx) ly, clamped to [0, 1]: every
 *         multiply and add rounded to fp32 on its own — F.interpolate(map, (h, w), mode="bilinear", align_corners=False)
 *         sampled straight from the raw cells, not through the 224-pixel crop
 *   k   = rint(255 v);  a8 = clamp(rint(weighted ? (256 alpha) v : 256 alpha), 0, 256)   (rint: half to even)
 *   out_c = (frame_c (256 - a8) + lut[k][c] a8 + 128) >> 8 */
int gcv_cam_overlay(const void* frames_u8_nhwc, int nframes, int H, int W, const int* boxes5, int n, const float* maps,
                    int mh, int mw, const unsigned char* lut768, float alpha, int weighted, void* out_u8_nhwc,
                    gcv_stream stream);

/* The way back of a whole-video scan: draw its result onto the frames — per crop row an outline of the face box with a
 * number tab in its corner, and along the bottom edge a timeline strip with a cursor at the frame's own place.  All marks
 * of a group of frames and the strip in one launch, one read and one write of the frames.
 *   frames    (nframes,H,W,3) uint8 RGB on the device, any byte alignment      out  the same shape; out == frames (in place)
 *             is allowed, and blocks that nothing touches are then not written
 *   frame_no  int32 device array of nframes: each frame's number on the timeline (read only where strip > 0)
 *   marks8    int32 device array of n rows (frame, top, right, bottom, left, colour, thick, label); frame counts the
 *             frames of this call
 *   timeline  (lanes, T) uint32 on the device; lanes, T, strip: see below.  strip == 0: no timeline, the three are ignored
 * Colours are packed r | g << 8 | b << 16; the top byte is ignored.  Everything is integer arithmetic (fixed, so that a CPU
 * restatement is bit-equal: tests/annotateutil.py); a / b is floor division of non-negative integers.  Pixel (f, y, x)
 * starts as p = frames[f][y][x] and goes through the following, later steps over earlier ones:
 *   marks     in row order.  A row takes part when frame == f, 0 <= top < bottom <= H, 0 <= left < right <= W,
 *             1 <= thick <= 16 and -1 <= label <= 999; any other row draws nothing.  A mark draws inside its box only
 *             (top <= y < bottom, left <= x < right):
 *               outline  p = colour when y - top < thick || bottom - 1 - y < thick || x - left < thick || right - 1 - x < thick
 *               tab      when label >= 0: nd = the number of decimal digits of label (1 ... 3); cy = (y - top) / thick,
 *                        cx = (x - left) / thick; the pixel is in the tab when cy < 7 && cx < 4 nd + 1 (the box clips the
 *                        tab; the tab is over the outline).  In the tab p = colour, unless the pixel is ink: 1 <= cy <= 5,
 *                        cx >= 1, gx = (cx - 1) % 4 < 3 and bit (cy - 1) * 3 + gx of FONT[digit (cx - 1) / 4 of label,
 *                        most significant first] set.  Ink is 0x000000 when (77 r + 150 g + 29 b) >> 8 >= 128 for the
 *                        mark's colour, else 0xFFFFFF.
 *               FONT     3 x 5 cells per digit, rows top to bottom, bit row * 3 + column:
 *                          0: 111 101 101 101 111    1: 010 110 010 010 111    2: 111 001 111 100 111    3: 111 001 111 001 111
 *                          4: 101 101 111 001 001    5: 111 100 111 001 111    6: 111 100 111 101 111    7: 111 001 001 001 001
 *                          8: 111 101 111 101 111    9: 111 101 111 001 111
 *   timeline  when strip > 0, over the marks: 1 <= lanes <= 8, lanes <= strip <= H, T >= 1, T W < 2^31.  For y >= H - strip:
 *               lane = ((y - (H - strip)) lanes) / strip;  t = (x T) / W;  p = timeline[lane T + t] & 0xFFFFFF
 *               cursor  c = frame_no[f]; if 0 <= c < T: x0 = (c W) / T, x1 = max(x0 + 1, ((c + 1) W) / T), and p = 0xFFFFFF
 *                       for x0 <= x < x1
 * Every pixel is read and written by one thread, so overlapping and nested marks are deterministic.  n == 0 && strip == 0
 * copies the frames (nothing is launched when in place).  Refused before anything is launched (gcv_last_error() says
 * why): nframes, H or W outside 1 ... 65536, nframes H W >= 2^31, n or strip negative, the timeline limits above.  The call
 * allocates, copies and synchronises nothing.  Not done here: text other than the number, anti-aliasing, video encoding. */
int gcv_scan_annotate(const void* frames_u8_nhwc, int nframes, int H, int W, const int* frame_no, const int* marks8, int n,
                      const unsigned* timeline, int lanes, int T, int strip, void* out_u8_nhwc, gcv_stream stream);

/* The decoder's and the encoder's side of a scan: YUV 4:2:0 frames as H.264 / HEVC decoders produce them, 1.5 bytes a
 * pixel, to the uint8 RGB frames every entry above reads (gcv_yuv420_to_rgb), and RGB frames back (gcv_rgb_to_yuv420).
 * One launch each, every byte read once and written once.
 *   yuv     nframes frames of 3 H W / 2 bytes each on the device, packed back to back (what a rawvideo pipe delivers):
 *             layout 0, i420: the Y plane H x W, then U (H/2) x (W/2), then V (H/2) x (W/2), each contiguous
 *             layout 1, nv12: the Y plane, then H/2 rows of W bytes U V U V ...
 *           frame f starts at byte f 3 H W / 2; the pointer may have any alignment
 *   rgb     (nframes,H,W,3) uint8 RGB on the device, any alignment
 *   matrix  0: bt601, (Kr, Kb) = (0.299, 0.114);  1: bt709, (0.2126, 0.0722);  Kg = 1 - Kr - Kb
 *   full_range  0: Y in 16 ... 235 and U, V in 16 ... 240 (limited);  otherwise 0 ... 255
 * The two buffers differ in size and must not overlap: neither call works in place.
 * Chroma siting: a chroma sample belongs to its 2 x 2 block of pixels — all four get it on the way in, it is the block's
 * mean on the way out.  Arithmetic (fixed and all-integer, so that a CPU restatement is bit-equal: tests/yuvutil.py);
 * int32, >> is an arithmetic shift, round(c 2^14) is round half up of the exact value:
 *   in     y' = Y - oy, oy = 16 (limited) or 0;  u' = U - 128;  v' = V - 128;  ky = 255/219 or 1, kc = 255/224 or 1
 *            R = clip((cy y' + crv v' + 8192) >> 14, 0, 255)             cy = round(ky 2^14), crv = round(kc 2 (1 - Kr) 2^14)
 *            G = clip((cy y' + cgu u' + cgv v' + 8192) >> 14, 0, 255)    cgu = round(-kc 2 (1 - Kb) Kb / Kg 2^14),
 *                                                                        cgv = round(-kc 2 (1 - Kr) Kr / Kg 2^14)
 *            B = clip((cy y' + cbu u' + 8192) >> 14, 0, 255)             cbu = round(kc 2 (1 - Kb) 2^14)
 *            (oy, cy, crv, cgu, cgv, cbu):  bt601 limited (16, 19077, 26149, -6419, -13320, 33050)
 *                                           bt601 full    (0, 16384, 22970, -5638, -11700, 29032)
 *                                           bt709 limited (16, 19077, 29372, -3494, -8731, 34610)
 *                                           bt709 full    (0, 16384, 25802, -3069, -7670, 30402)
 *   out    Y = oy + ((ar R + ag G + ab B + 8192) >> 14);  s = 219/255 or 1;  ar = round(Kr s 2^14), ab = round(Kb s 2^14),
 *            ag = round(s 2^14) - ar - ab, so that white gives 235 / 255 exactly
 *          with (Sr, Sg, Sb) the sums over the block's four pixels, 0 ... 1020, and t = 224/255 or 1:
 *            U = clip(128 + ((ur Sr + ug Sg + ub Sb + 32768) >> 16), 0, 255)   ur = round(-Kr / (2 (1 - Kb)) t 2^14), ub = round(t 2^13)
 *            V = clip(128 + ((vr Sr + vg Sg + vb Sb + 32768) >> 16), 0, 255)   vr = round(t 2^13), vb = round(-Kb / (2 (1 - Kr)) t 2^14)
 *            ug = -ur - ub and vg = -vr - vb, so that grey gives 128 exactly
 *            (oy, ar, ag, ab; ur, ug, ub; vr, vg, vb):
 *              bt601 limited (16, 4207, 8260, 1604; -2428, -4768, 7196; 7196, -6026, -1170)
 *              bt601 full    (0, 4899, 9617, 1868; -2765, -5427, 8192; 8192, -6860, -1332)
 *              bt709 limited (16, 2991, 10064, 1016; -1649, -5547, 7196; 7196, -6536, -660)
 *              bt709 full    (0, 3483, 11718, 1183; -1877, -6315, 8192; 8192, -7441, -751)
 * Refused before anything is launched (gcv_last_error() says why): H or W odd or outside 2 ... 65536, a layout or matrix
 * other than 0 and 1, nframes negative, nframes H W >= 2^31, a null pointer with nframes > 0.  nframes == 0 launches
 * nothing.  The calls allocate, copy and synchronise nothing.
 * Not done here: interpolated (co-sited) chroma, 4:2:2 / 4:4:4 / 10-bit formats, bt2020, bit-equality with any third-party
 * converter. */
int gcv_yuv420_to_rgb(const void* yuv_u8, int nframes, int H, int W, int layout, int matrix, int full_range,
                      void* rgb_u8_nhwc, gcv_stream stream);
int gcv_rgb_to_yuv420(const void* rgb_u8_nhwc, int nframes, int H, int W, int layout, int matrix, int full_range,
                      void* yuv_u8, gcv_stream stream);

/* Follow a face between two detector frames: integer block matching of n (track, skipped frame) jobs in one launch.
 * A whole-video scan runs its CPU face detector on every k-th frame; in a skipped frame the face is searched around the
 * interpolated ("prior") box, with the two detected faces around the gap as templates.
 *   frames  (nframes,H,W,3) uint8 RGB on the device, as for gcv_face_crop_resize
 *   jobs17  int32 device array of n rows:
 *             fs, top, right, bottom, left      the skipped frame and the prior box in it
 *             fa, ta, ra, ba, la, wa            anchor a: the detection before the gap, and its weight
 *             fb, tb, rb, bb, lb, wb            anchor b: the detection after the gap, and its weight
 *   grid    G: 16, 32 or 64 cells a side;  radius R: 0 ... 32 cells of search range either way
 *   out4    (n,4) int32: (oy, ox, best cost, cost at zero displacement); (oy, ox) is the pixel offset to add to the prior
 *           box, whose size does not change
 * Arithmetic (fixed and all-integer, so that a CPU restatement is bit-equal: tests/followutil.py); a // b is floor
 * division, also for negative a:
 *   luma of a pixel   Y = (77 R + 150 G + 29 B + 128) >> 8
 *   cell edges        for an extent h: e_h(u) = (u h) // G for any integer u; cell u covers the rows [e_h(u), e_h(u + 1))
 *                     relative to the box top; columns alike with w
 *   precondition      h >= G and w >= G for the prior box and both anchors, so that no cell is empty
 *   cell value        (sum of Y over the cell's pixel rectangle + cnt // 2) // cnt, cnt the rectangle's pixels: 0 ... 255
 *   templates         A[u][v], B[u][v], u, v in [0, G): anchor a's box in frame fa and anchor b's box in frame fb, each
 *                     with its own height and width — a face that grows or shrinks across the gap is compared at a
 *                     normalised scale
 *   search window     V[u][v], u, v in [-R, G + R): frame fs around the prior box, with the prior box's h, w
 *   displacements     (dy, dx) in [-R, R]^2 count cells, so the search range scales with the face
 *   cost(dy, dx)      sum over u, v of wa |A[u][v] - V[u + dy][v + dx]| + wb |B[u][v] - V[u + dy][v + dx]|
 *   valid candidate   0 <= top + e_h(dy) and top + e_h(dy) + h <= H, and the same in x.  e_h(G + dy) = h + e_h(dy), so the
 *                     cells dy ... dy + G - 1 tile exactly the displaced box: a valid candidate reads only pixels inside the
 *                     frame, (0, 0) is always valid, and window cells no valid candidate uses are never read
 *   result            the valid candidate with the smallest (cost, dy dy + dx dx, dy, dx) in lexicographic order:
 *                     out = (e_h(dy), e_w(dx), cost(dy, dx), cost(0, 0))
 * Refused before anything is launched (gcv_last_error() says why): grid not 16, 32 or 64; radius outside 0 ... 32;
 * nframes, H or W not positive (or H W > 2^30).  n == 0 launches nothing.  The rows are the caller's to check (the Python
 * binding does): frame indices in range, boxes inside the frame, every h, w >= G, wa, wb >= 0 and 1 <= wa + wb <= 1024, which
 * keeps the cost below 2^31 (64 * 64 * 255 * 1024).  A row that breaks any of this reads nothing and gives (0, 0, 0, 0).
 * One launch, one workgroup per job; the call allocates, copies and synchronises nothing.
 * Not done here: sub-cell refinement, a change of box size inside a gap beyond the interpolation.  Extending a track past
 * its first and last detection is gcv_track_chain's. */
int gcv_track_match(const void* frames_u8_nhwc, int nframes, int H, int W, const int* jobs17, int n, int grid, int radius,
                    int* out4, gcv_stream s);

/* Carry a face past its first or last detection: n chains in one launch, each a walk over consecutive frames in which
 * every step searches around the box the step before found.  gcv_track_match cannot do this — each of its jobs needs a
 * prior box that is known before the launch.
 *   frames  (nframes,H,W,3) uint8 RGB on the device, as for gcv_track_match
 *   jobs11  int32 device array of n rows:
 *             fa, top, right, bottom, left   the template: a detected box in frame fa; its h = bottom - top and
 *                                            w = right - left are the size of every box of the chain
 *             fs, dir, steps                 the frames searched are fs, fs + dir, ..., fs + dir (steps - 1); dir is +1 or
 *                                            -1; 1 <= steps <= max_steps
 *             py, px                         the pixel offset of the prior box of the first step from the template box: 0, 0
 *                                            for a chain that starts at the detection; the sum of the (oy, ox) rows of an
 *                                            earlier launch for a chain that continues it
 *             stop                           a cost bound, 0 ... 2^31 - 1
 *   max_steps  1 ... 1024: the rows of out4 per job
 *   grid, radius  as for gcv_track_match
 *   out4    (n,max_steps,4) int32: (oy, ox, cost, cost0) per step; (oy, ox) is relative to that step's prior box — the
 *           caller adds the steps up
 * Arithmetic: gcv_track_match's luma, cell edges, cell values and validity, and its minimum over
 * (cost, dy dy + dx dx, dy, dx).  With A[u][v] the cells of the template box in frame fa, step k = 0 ... steps - 1 is:
 *   prior box         step 0: the template box shifted by (py, px); step k: the prior of step k - 1 shifted by its (oy, ox)
 *   search window     V[u][v], u, v in [-R, G + R): frame fs + dir k around that prior, with the template's h and w
 *   cost(dy, dx)      sum over u, v of |A[u][v] - V[u + dy][v + dx]|, over the valid candidates of that prior
 *   result            out[k] = (e_h(dy), e_w(dx), cost(dy, dx), cost(0, 0)) of the smallest (cost, dy dy + dx dx, dy, dx)
 *   stop              if that smallest cost exceeds stop (cost > stop), step k and every later step of the job write
 *                     (0, 0, -1, -1) and the job ends there; so do the rows steps ... max_steps - 1
 * The template is not updated along the chain, so position errors do not accumulate in it; a face that changes pose or
 * exposure makes the cost rise.  Each step equals gcv_track_match on the row (frame, prior box, template, 1, template, 0)
 * — both anchors the template, weighted 1 and 0 —, which is how tests/extendutil.py restates it.
 * Refused before anything is launched (gcv_last_error() says why): grid not 16, 32 or 64; radius outside 0 ... 32;
 * max_steps outside 1 ... 1024; nframes, H or W not positive (or H W > 2^30).  n == 0 launches nothing.  The rows are the
 * caller's to check (the Python binding does): fa and every searched frame in range, the template box and the first prior
 * box inside the frame, h, w >= G, dir = +-1, 1 <= steps <= max_steps, stop >= 0.  A row that breaks any of this reads
 * nothing and writes (0, 0, -1, -1) throughout.
 * One launch, one workgroup per chain; the template's cells stay in LDS for the whole chain.  A launch of a few dozen
 * chains is latency-bound: steps x the latency of one step.  The call allocates, copies and synchronises nothing.
 * Not done here: a change of box size along a chain, sub-cell refinement, template update. */
int gcv_track_chain(const void* frames_u8_nhwc, int nframes, int H, int W, const int* jobs11, int n, int max_steps, int grid,
                    int radius, int* out4, gcv_stream s);

/* Shot cuts: per-region luma histograms of every frame (gcv_frame_hist) and their L1 distance between consecutive frames
 * (gcv_hist_diff).  A whole-video scan links face boxes into tracks by position; after a hard cut the face of another
 * person often sits where the last one sat.  pred_func.shot_cuts turns the distances into cuts, at which tracks end.
 *   frames   (nframes,H,W,3) uint8 RGB on the device, as for gcv_face_crop_resize; the pointer may have any alignment (a
 *            slice frames[1:] of a 37 x 53 video starts 5 883 bytes in), and no byte outside
 *            [frames, frames + nframes H W 3) is read
 *   regions  R: 1, 2, 4 or 8; a frame is cut into R x R regions
 *   hist     (nframes, R R, 64) uint32: hist[f][u R + v][b] = the number of pixels of region (u, v) of frame f in bin b.
 *            Every element is written, empty bins as 0.  The counts of a region add up to its pixel count
 *   dist     (nframes - 1, R R) uint32: dist[p][r] = sum over b of |hist[p + 1][r][b] - hist[p][r][b]|, at most twice the
 *            region's pixel count (<= 2^31)
 * Arithmetic (fixed and all-integer, so that a CPU restatement is bit-equal: tests/cutsutil.py); a // b is floor division:
 *   region (u, v)     rows [(u H) // R, ((u + 1) H) // R) and columns [(v W) // R, ((v + 1) W) // R): the cell-edge rule of
 *                     gcv_track_match.  H >= R and W >= R, so no region is empty
 *   luma of a pixel   Y = (77 R + 150 G + 29 B + 128) >> 8, as in gcv_track_match;  bin = Y >> 2: 64 bins
 * Refused before anything is launched (gcv_last_error() says why): regions not 1, 2, 4 or 8; nframes, H or W not positive;
 * H < regions or W < regions; H W > 2^30 (a count is 32 bits); a null pointer.  gcv_hist_diff with nframes == 1 launches
 * nothing and writes nothing.
 * gcv_frame_hist reads every pixel once: one workgroup per (frame, region), or, where that leaves the chip idle (few
 * frames, R = 1 or 2), several per region whose counts are merged by integer atomic adds into the output, which a
 * hipMemsetAsync on the stream zeroes first — integer adds commute, so the result is the same whatever the order.
 * gcv_hist_diff is one launch.  Neither call allocates, copies or synchronises anything.
 * Not done here: fades and dissolves (only a hard cut changes every region at once; the three entries below are for
 * those), and two shots whose regions have the same luma distribution are not told apart. */
int gcv_frame_hist(const void* frames_u8_nhwc, int nframes, int H, int W, int regions, uint32_t* hist_u32,
                   gcv_stream stream);
int gcv_hist_diff(const uint32_t* hist_u32, int nframes, int regions, uint32_t* dist_u32, gcv_stream stream);

/* Fades and dissolves: luma sums on a grid of cells (gcv_frame_cells), the least-squares sums of every frame of a span
 * against the line between the span's two ends (gcv_blend_fit), and the histogram distance between those ends
 * (gcv_hist_diff_lag).  A linear dissolve makes every frame between its ends a pixelwise blend (1 - a) A + a B, so the
 * cell vector of a middle frame lies on the straight line between the cell vectors of the ends; motion, cuts and flashes
 * leave that line.  pred_func.shot_transitions turns the sums into transitions, whose frames a scan keeps out of tracks.
 *   frames   as for gcv_frame_hist: any alignment, and no byte outside [frames, frames + nframes H W 3) is read
 *   grid     G: 8, 16 or 32; a frame is cut into G x G cells
 *   cells    (nframes, G G) uint32: cells[f][u G + v] = the sum of Y over the pixels of cell (u, v) of frame f.  Every
 *            element is written
 *   lag      L: the span p has the ends p and p + L.  gcv_blend_fit: 2 ... 32; gcv_hist_diff_lag: any L >= 1
 *   fit      (nframes - L, 2 L - 1) int64; with A = cells[p], B = cells[p + L], D = B - A and M_k = cells[p + k] - A for
 *            k = 1 ... L - 1 (differences of integers, signed), the row p is
 *              [ Sdd, Smd_1 ... Smd_(L-1), Smm_1 ... Smm_(L-1) ],
 *              Sdd = sum over the cells of D D,  Smd_k = sum of M_k D,  Smm_k = sum of M_k M_k
 *            The least-squares position of frame p + k on the line is a_k = Smd_k / Sdd, and its squared distance from the
 *            line, relative to the line's squared length, rho_k = (Smm_k - Smd_k^2 / Sdd) / Sdd — the caller's to compute, in
 *            floating point (Smd_k^2 does not fit 64 bits)
 *   dist     (nframes - L, R R) uint32: dist[p][r] = sum over b of |hist[p + L][r][b] - hist[p][r][b]|; L = 1 is
 *            gcv_hist_diff
 * Arithmetic (fixed and all-integer, so that a CPU restatement is bit-equal: tests/transutil.py); a // b is floor division:
 *   cell (u, v)       rows [(u H) // G, ((u + 1) H) // G) and columns [(v W) // G, ((v + 1) W) // G), the region rule of
 *                     gcv_frame_hist.  H >= G and W >= G, so no cell is empty
 *   luma of a pixel   Y = (77 R + 150 G + 29 B + 128) >> 8, as above
 *   the sums          exact in int64 whenever every row of cells has a sum of squares below 2^62: then Sdd <= |A|^2 + |B|^2
 *                     < 2^63 (the entries are non-negative), Smm_k alike, and |Smd_k| <= sqrt(Smm_k Sdd) < 2^63.  Rows
 *                     from gcv_frame_cells meet this: a side of a cell is ceil(H / G) < 2 H / G pixels at most, so a cell
 *                     holds n < 4 H W / G^2 <= H W / 16 of them, and the sum of squares of a row is at most
 *                     255^2 max(n) sum(n) < 255^2 (H W)^2 / 16 <= 65025 * 2^46 < 2^62 for H W <= 2^25 — the bound
 *                     gcv_frame_cells enforces (a cell is then below 2^29, and fits 32 bits with room to spare).  Rows
 *                     from elsewhere are the caller's to check
 * Refused before anything is launched (gcv_last_error() says why): grid not 8, 16 or 32; nframes, H or W not positive;
 * H < grid or W < grid; H W > 2^25; lag outside 2 ... 32 (blend fit) or below 1 (hist diff); regions not 1, 2, 4 or 8; a
 * null pointer.  gcv_blend_fit and gcv_hist_diff_lag with nframes <= lag launch nothing, write nothing and return 0.
 * gcv_frame_cells reads every pixel once: one workgroup per row of G cells of a frame, or, where that leaves the chip idle
 * (few frames), several per row, merged by integer atomic adds into the output, which a hipMemsetAsync on the stream
 * zeroes first.  gcv_blend_fit is one launch, a workgroup per span; gcv_hist_diff_lag is gcv_hist_diff's kernel.  None of
 * the calls allocates, copies or synchronises anything.
 * Not done here: non-linear (eased) dissolves, wipes, and telling a slow pan from a blend — the cells of a slow pan are
 * close to linear too, which is why pred_func.shot_transitions also asks the ends of a span to differ in gcv_hist_diff_lag. */
int gcv_frame_cells(const void* frames_u8_nhwc, int nframes, int H, int W, int grid, uint32_t* cells_u32,
                    gcv_stream stream);
int gcv_blend_fit(const uint32_t* cells_u32, int nframes, int grid, int lag, int64_t* fit_i64, gcv_stream stream);
int gcv_hist_diff_lag(const uint32_t* hist_u32, int nframes, int regions, int lag, uint32_t* dist_u32, gcv_stream stream);

/* Is a face crop usable: sharpness, gradient and exposure sums of n face boxes in one launch.  A whole-video scan scores
 * every face of every frame; a face smeared by motion or defocus, blown out by a flash or lost in the dark still gets a
 * crop, a score and a vote.  pred_func.face_quality turns the sums into per-box measures and pred_func.quality_keep into
 * the rows a scan drops: the policy stays in Python, the numbers are returned.
 *   frames  (nframes,H,W,3) uint8 RGB on the device, as for gcv_face_crop_resize; the pointer may have any alignment, and
 *           no byte outside [frames, frames + nframes H W 3) is read
 *   boxes5  int32 device array of n rows (frame, top, right, bottom, left), as for gcv_face_crop_resize
 *   grid    G: 16, 32 or 64 cells a side
 *   out8    (n,8) int64: (G, S1, S2, L2, GX, GY, dark, bright)
 * Arithmetic (fixed and all-integer, so that a CPU restatement is bit-equal: tests/qualityutil.py); a // b is floor
 * division.  Luma, cell edges and cell value are gcv_track_match's, with h = bottom - top and w = right - left:
 *   luma of a pixel   Y = (77 R + 150 G + 29 B + 128) >> 8
 *   cell edges        e_h(u) = (u h) // G; cell (u, v), u, v in [0, G), covers the rows [top + e_h(u), top + e_h(u + 1)) and
 *                     the columns [left + e_w(v), left + e_w(v + 1)): the cells tile the box exactly
 *   precondition      h >= G and w >= G, so that no cell is empty
 *   cell value        c[u][v] = (sum of Y over the cell's pixel rectangle + cnt // 2) // cnt, cnt the rectangle's pixels:
 *                     0 ... 255
 *   S1                sum over all cells of c                                          <= 255 G^2 <= 1.1e6
 *   S2                sum over all cells of c^2                                        <= 255^2 G^2 <= 2.7e8
 *   L2                sum over the interior u, v in [1, G - 1) of
 *                     (4 c[u][v] - c[u-1][v] - c[u+1][v] - c[u][v-1] - c[u][v+1])^2    <= 62^2 1020^2 ~ 4.0e9: past a signed
 *                     32 bits, hence int64 outputs; 16 terms (a lane's, at G = 64) stay below 2^24, a wave's below 2^31
 *   GX                sum over u in [0, G), v in [0, G - 1) of (c[u][v+1] - c[u][v])^2   <= 255^2 G (G - 1) <= 2.7e8
 *   GY                sum over u in [0, G - 1), v in [0, G) of (c[u+1][v] - c[u][v])^2   <= 2.7e8
 *   dark, bright      the number of cells with c < 16, and with c > 239
 * L2 is the energy of the discrete Laplacian, which blur removes first; GX against GY tells the direction of a motion blur
 * (a horizontal smear lowers GX, the differences along a row, and leaves GY).  All of it is relative to the cell: blur
 * finer than a cell (h / G by w / G pixels) is invisible, so the grid should follow the face size.
 * A bad row — a frame index out of range, a box outside the frame, h or w below G — reads nothing and gives eight zeros:
 * out[0] == 0 marks it (a good row has out[0] == G).  The Python binding refuses such rows instead.
 * Refused before anything is launched (gcv_last_error() says why): grid not 16, 32 or 64; nframes, H or W not positive;
 * H W > 2^30 (a cell's sum is 32 bits); a null pointer with n > 0.  n == 0 launches nothing and writes nothing.
 * One launch, one workgroup of 256 threads per box; the call allocates, copies and synchronises nothing.
 * Not done here: any judgement (thresholds are the caller's), blur finer than a cell, a per-box choice of the grid, colour
 * casts and compression artefacts. */
int gcv_face_quality(const void* frames_u8_nhwc, int nframes, int H, int W, const int* boxes5, int n, int grid,
                     int64_t* out8, gcv_stream stream);

/* Who is it: an appearance signature of n face boxes in one launch (gcv_face_signature), and for every pair of tracks the
 * distance of their two most alike crops (gcv_sig_link).  A whole-video scan ends a track at every cut and at both ends of
 * every dissolve, so edited footage comes back as many short tracks; position cannot link them across a cut, appearance
 * can.  pred_func.link_tracks turns the distances into persons: the policy stays in Python, the numbers are returned.
 *   frames   (nframes,H,W,3) uint8 RGB on the device, as for gcv_face_quality; the pointer may have any alignment, and no
 *            byte outside [frames, frames + nframes H W 3) is read
 *   boxes5   int32 device array of n rows (frame, top, right, bottom, left), as for gcv_face_quality
 *   sig384   (n,384) uint8, every row: bytes 0 ... 255 the normalised luma N[u][v] of a 16 x 16 grid, 256 ... 319 Cb of an
 *            8 x 8 grid, 320 ... 383 Cr of the same grid, each row-major
 * Arithmetic of the signature (fixed and all-integer, so that a CPU restatement is bit-equal: tests/personutil.py); a // b
 * is floor division, of non-negative integers throughout; h = bottom - top, w = right - left:
 *   cell edges        16-grid: ey[i] = (i h) >> 4, ex[i] = (i w) >> 4, i = 0 ... 16; 8-grid: (i h) >> 3, (i w) >> 3, i = 0 ... 8.
 *                     Cell (u, v) covers the rows [top + ey[u], top + ey[u + 1]) and the columns [left + ex[v],
 *                     left + ex[v + 1]).  (i h) >> 3 = (2 i h) >> 4: a cell of the 8-grid is four cells of the 16-grid
 *   precondition      h >= 16 and w >= 16, so that no cell is empty
 *   luma cells        c[u][v] on the 16-grid: gcv_track_match's cell value, (sum of Y + cnt // 2) // cnt with
 *                     Y = (77 R + 150 G + 29 B + 128) >> 8
 *   normalisation     cancels the gain and the offset of a shot's exposure.  S1 = sum of c over the 256 cells,
 *                     d = 256 c - S1 (256 times the distance from the mean, exactly), A = sum of |d|;
 *                     N = clamp(128 + sgn(d) ((8192 |d| + A // 2) // A), 0, 255), and N = 128 everywhere when A == 0.
 *                     |d| <= 65280 and A <= 256 * 65280, so 8192 |d| + A // 2 < 2^31
 *   chroma cells      per pixel Cb = (32896 - 43 R - 85 G + 128 B) >> 8 and Cr = (32896 + 128 R - 107 G - 21 B) >> 8, both
 *                     in [1, 256], 256 only for the pixel (0, 0, 255) resp. (255, 0, 0).  The cell on the 8-grid is
 *                     min((sum + cnt // 2) // cnt, 255): the minimum matters only for a cell of nothing but that pixel
 * A bad row — a frame index out of range, a box outside the frame, h or w below 16 — reads nothing and gives 384 zero bytes
 * (a good row never does: the luma bytes of a good row average 128).  The Python binding refuses such rows instead.
 * Refused before anything is launched (gcv_last_error() says why): nframes, H or W not positive; H W > 2^28 (a chroma
 * cell's sum is 32 bits); a null pointer with n > 0.  n == 0 launches nothing and writes nothing.
 * One launch, one workgroup of 256 threads per box; the call allocates, copies and synchronises nothing.
 *
 *   sig      (n,384) uint8 on the device, 16-byte aligned: rows as above (any bytes will do: the distance is plain L1)
 *   owner    int32 device array of n: the track of each row, in [0, T); -1 — or anything else outside [0, T) — for a row
 *            that takes no part.  Need not be sorted
 *   out      (T,T) uint32: out[a][b] = the minimum over the rows i of track a and the rows j of track b, a != b, of
 *            sum over k = 0 ... 383 of |sig[i][k] - sig[j][k]|, at most 384 * 255 = 97 920.  Symmetric.  The diagonal, and
 *            every pair one of whose tracks has no row, hold 0xFFFFFFFF.  Every element is written
 * Refused: n outside 0 ... 65 536, T outside 0 ... 4 096, a null or misaligned pointer (n, T > 0).  n == 0 or T == 0
 * launches nothing and writes nothing.  Otherwise a hipMemsetAsync on the stream sets out to 0xFF bytes and one launch
 * follows: a workgroup per pair of 64-row tiles, the minima merged into out by unsigned integer atomic minima, whose
 * result does not depend on their order.  The call allocates, copies and synchronises nothing.
 * Not done here: any judgement (the threshold is the caller's), alignment of the face inside its box beyond what the
 * detector gives, and any claim about real faces — the signature is a coarse picture of the box, not an identity
 * embedding. */
int gcv_face_signature(const void* frames_u8_nhwc, int nframes, int H, int W, const int* boxes5, int n, void* sig384,
                       gcv_stream stream);
int gcv_sig_link(const void* sig384, const int* owner, int n, int tracks, uint32_t* out_u32, gcv_stream stream);

/* pred_vid's reduction (model/pred_func.py:120,125): mean2[c] = mean_r sigmoid(logits[r][c]). */
int gcv_vote(const float* logits, int rows, float* mean2, gcv_stream stream);

/* Row N3: the same vote for several videos batched into ONE forward.  logits rows are [net 0 frames 0..B-1; net 1 ...]
 * (model/genconvit.py:74); video v owns frames [offsets[v], offsets[v+1]) (int32 device array of n_videos+1 entries);
 * mean2[v][c] = mean over its frames and nets of sigmoid(logit[.][c]) — what max_prediction_value reduces per video. */
int gcv_vote_segments(const float* logits, int batch, int nets, const int* offsets, int n_videos, float* mean2,
                      gcv_stream stream);

/* Per-frame scores and votes over arbitrary ranges of frame rows, for sliding windows over a face track.  logits as for
 * gcv_vote_segments ([net 0 frames 0..batch-1; net 1 ...], two columns, nets = 1 or 2).
 *   frame_p (batch,2) fp32, required: frame_p[f][c] = (1/nets) sum_n sigmoid(logits[n batch + f][c]) — the timeline
 *   ranges2 int32 device array of n_ranges rows [lo, hi) of frame rows; they may overlap, nest, repeat, come unsorted;
 *           a row is clamped to [0, batch] (a caller should reject what that would change, as the Python binding does)
 *   mean2   (n_ranges,2) fp32: mean2[k][c] = mean of frame_p[lo..hi-1][c] = the mean over the range's frames and nets of
 *           sigmoid(logit) that max_prediction_value reduces; 0.5 for an empty range, like gcv_vote_segments, with which
 *           it agrees (to fp32 summation order) on a range that is one of its segments
 * Two small launches on `stream`: every sigmoid is evaluated once, in the frame pass; the range pass reads frame_p.
 * n_ranges == 0 (ranges2 and mean2 may be null) fills frame_p only. */
int gcv_vote_windows(const float* logits, int batch, int nets, const int* ranges2, int n_ranges, float* frame_p,
                     float* mean2, gcv_stream stream);

/* ---- multi-GPU: frame shards, one process per GPU, RCCL over xGMI (new capability: the reference is single
 * device, model/pred_func.py:15).  The only exchange of the path is one all-gather of per-frame logits before the
 * vote.  RCCL is bound at run time (dlopen: $GCV_RCCL_PATH, an already loaded librccl, then
 * /opt/rocm/lib) so that the library shares the process's RCCL the way it shares its HIP runtime.
 *   gcv_comm_available : 1 when RCCL and its entry points could be bound in this process (dlopen + dlsym only), else 0
 *                        with the reason in gcv_last_error(): the cheap probe every rank runs before the collective
 *   gcv_comm_count     : ranks in the communicator as RCCL reports them (ncclCommCount)
 *   gcv_comm_unique_id : rank 0 fills 128 bytes (ncclUniqueId); the caller ships them to every rank (any channel)
 *   gcv_comm_create    : collective over all `world` ranks (ncclCommInitRank) on `device`
 *   gcv_allgather_logits: all[r * n_local .. (r+1) * n_local) = rank r's `local` (n_local floats, equal on all
 *                        ranks: pad ragged shards), enqueued on `stream`; world = 1 is a device copy */
typedef struct gcv_comm gcv_comm;
int  gcv_comm_available(void);
int  gcv_comm_count(gcv_comm* c);
int  gcv_comm_unique_id(void* id128);
int  gcv_comm_create(gcv_comm** c, int world, int rank, const void* id128, int device);
void gcv_comm_destroy(gcv_comm* c);
int  gcv_allgather_logits(gcv_comm* c, const float* local, int n_local, float* all, gcv_stream stream);

/* Per-launch timing with HIP events on the launch stream.  After gcv_profile_enable(h,1) every
 * kernel launch of the following forwards is bracketed by events; gcv_profile_report() waits for
 * them and returns a JSON array aggregated by op tag (launches, ms, algorithmic flops / bytes)
 * and clears the records.  The returned string lives until the next call on the handle.  While profiling is on, every
 * tagged launch is also a roctx range of the same name (roctxRangePushA / roctxRangePop, bound at run time from
 * librocprofiler-sdk-roctx / libroctx64 when present), so `rocprofv3 --marker-trace --kernel-trace` groups kernels by op. */
int gcv_profile_enable(gcv_handle* h, int on);
const char* gcv_profile_report(gcv_handle* h);

/* ---- taps: named intermediates of the forwards, copied into caller-owned device buffers (tests) ----
 * gcv_tap_set registers `dst` (`bytes` long) for tap `name` on the handle; dst == NULL removes it.  Each following
 * gcv_ed_forward / gcv_vae_forward / gcv_genconvit_forward of the handle enqueues a hipMemcpyAsync device-to-device
 * of the tensor into `dst` on the stream that produced it (the VAE's side stream for backbone(x) under the split
 * schedule), ordered before the forward's end on `stream` like the rest of its work.  With no tap set nothing is
 * copied, launched or synchronised.  An unknown name is an error of gcv_tap_set; a buffer whose size differs from the
 * tensor's size at the forward's batch makes the forward fail.
 * gcv_tap_written: 1 if the last forward of the tap's network stored the whole tensor, 0 if the dispatch never stores
 * it in HBM for some segment (then `dst` holds stale data), < 0 if no such tap is set.  Example: the residual stream
 * after the last block of stage 0 / 1 when that block's MLP epilogue applies the stage boundary's LayerNorm-patchify.
 * Layouts (T = the handle's storage dtype; NHWC = (B, H, W, C) row-major; B = the forward's batch):
 *   ed.e1..ed.e5      encoder outputs, NHWC T: 112x112x16, 56x56x32, 28x28x64, 14x14x128, 7x7x256
 *   ed.d1..ed.d4      decoder outputs, NHWC T: 14x14x128, 28x28x64, 56x56x32, 112x112x16;  ed.rec: 224x224x3 NHWC T
 *   ed.feat           (B, 2000) T: GELU(cat(backbone(rec), backbone(x))), the input of the head's fc
 *   vae.v1..vae.v4    encoder outputs, NHWC T: 112x112x16, 56x56x32, 28x28x64, 14x14x128
 *   vae.mu            (B, 12544) fp32 in the reference's order (c * 49 + hw);  vae.z: the sample z, NHWC T 7x7x256
 *   vae.d1..vae.d3    decoder outputs, NHWC T: 14x14x64, 28x28x32, 56x56x16;  vae.xhat: 112x112x3 NHWC T
 *   vae.feat          (B, 2000) T: ReLU(cat(backbone(x), backbone(x_hat)))
 *   <net>.bb.<t>      the ConvNeXt-T token stream of network <net> (ed, vae), its segments concatenated in the order
 *                     ed: [backbone(rec) B images, backbone(x) B images], vae: [backbone(x) @224, backbone(x_hat) @112],
 *                     whichever launches ran them.  Per segment, images in order, tokens (h, w) row-major, channels
 *                     innermost, in T, with h = H/4 >> i, w = W/4 >> i at stage i (H = W = 224 or 112):
 *     stem            (tokens, 96) after the stem's LayerNorm
 *     s<i>.b<j>       (tokens, C_i) the residual stream after block j of stage i (C = 96, 192, 384, 768; j < 3, 3, 9, 3)
 *     s<i>.down_in    i = 1..3: the operand of stage i's downsample GEMM, (h_i * w_i rows, 4 * C_(i-1)) with
 *                     (dy, dx, c) innermost: LayerNorm2d + 2x2 patch rows of stage i-1's output, whichever kernel wrote it
 *     pool            (images, 768) the pooled + LayerNorm'ed rows */
int gcv_tap_set(gcv_handle* h, const char* name, void* dst, size_t bytes);
int gcv_tap_clear(gcv_handle* h);
int gcv_tap_written(gcv_handle* h, const char* name);

/* ---- per-kernel entry points (unit parity tests; same kernels the forwards launch) ---- */
enum { GCV_A_PLAIN = 0, GCV_A_IM2COL3_POOL = 1, GCV_A_IM2COL3_S2 = 2 };
enum { GCV_EPI_BIAS_ACT = 0, GCV_EPI_RESID = 1, GCV_EPI_POOL4 = 2, GCV_EPI_CONVT = 3, GCV_EPI_SPLITK = 4 };

typedef struct {
  const void* A; const void* Wt; void* C;
  const float* bias; const float* gamma; const void* resid; float* partial;
  int M, N, K, lda, ldc, act, splitk, k_per_split, H, W, cin_log2, cout_log2;
} gcv_gemm_args;

/* C = epilogue(A * Wt^T): nn.Linear / Conv2d-as-GEMM / ConvTranspose2d(k=s=2) / split-K slab */
int gcv_k_gemm(int dtype, int a_mode, int epi, const gcv_gemm_args* a, gcv_stream s);
/* Test query: the kernel and grid that gcv_k_gemm picks for the launch *a.  The pointers in *a are tested for null and
 * alignment only, never dereferenced.  out10 = {kind, five tile fields, grid.x, grid.y, threads per workgroup, dynamic LDS
 * bytes}; or the launcher's error.  The tile fields by kind:
 *   0 tile GEMM         BM, BN (workgroup tile), WM, WN (wave tile), BKB (bytes per LDS row: a K tile of BKB / sizeof(T))
 *   1 LDS-DMA GEMM      128, 192, 64, 96, BKB (64 or 128)
 *   2 direct 3x3 conv   CIN (16 / 32), STRIDE (1: conv + ReLU + 2x2 max-pool, 2: stride-2 conv + LeakyReLU), 0, 0, 0
 * No HIP call: works without a GPU. */
int gcv_gemm_plan(int dtype, int a_mode, int epi, const gcv_gemm_args* a, int* out10);
int gcv_k_stem_ln(int dtype, const void* x, int64_t sb, int64_t sc, int64_t sy, int64_t sx, const float* wp,
                  const float* bias, const float* lnw, const float* lnb, void* out, int nimg, int Ho, int Wo,
                  float eps, gcv_stream s);
/* the stem at output width C: 96 (ConvNeXt-T, = gcv_k_stem_ln) or 192 (ConvNeXt-L); wp [48][C] */
int gcv_k_stem_ln_c(int dtype, const void* x, int64_t sb, int64_t sc, int64_t sy, int64_t sx, const float* wp,
                    const float* bias, const float* lnw, const float* lnb, void* out, int nimg, int Ho, int Wo, int C,
                    float eps, gcv_stream s);
int gcv_k_dwconv7_ln(int dtype, const void* x, const float* wdw, const float* bdw, const float* lnw,
                     const float* lnb, void* y, int nimg, int H, int W, int C, float eps, gcv_stream s);
/* The same on two image groups of one C, (x0, y0): nimg0 maps of H0 x W0 and (x1, y1): nimg1 maps of H1 x W1, in ONE launch
 * where the two kernels gcv_dw_plan names for them have a merged form (group 0 the wider map: mfma or roll 96x56 + roll
 * 96x28, roll 192x28 + 192x14, roll 384x14 + 384x7, roll 768x7 + tiny 768x3x3; the VAE's 224- + 112-pixel pass), in two
 * launches otherwise.  Each group keeps its gcv_dw_plan; the outputs are bit for bit those of two gcv_k_dwconv7_ln calls. */
int gcv_k_dwconv7_ln2(int dtype, const void* x0, void* y0, int nimg0, int H0, int W0, const void* x1, void* y1,
                      int nimg1, int H1, int W1, const float* wdw, const float* bdw, const float* lnw, const float* lnb,
                      int C, float eps, gcv_stream s);
/* Test query: the kernel and grid that gcv_k_dwconv7_ln picks for nimg H x W x C images, x and y 16-byte aligned or not.
 * out5 = {kind (0 tile, 1 tiny, 2 tiny-pair, 3 roll, 4 mfma, 5 pair), workgroups, threads per workgroup, dynamic LDS bytes,
 * rows per band (roll, mfma, pair; else 0)}; or the launcher's error.  No HIP call: works without a GPU. */
int gcv_dw_plan(int dtype, int nimg, int H, int W, int C, int aligned, int* out5);
/* Test entries: gcv_k_dwconv7_ln / gcv_k_dwconv7_ln2 on nimg images under the plan of a launch of plan_nimg images (<= 0: of
 * nimg).  The kernel and the rows per band are those gcv_dw_plan reports for plan_nimg images, the grid covers nimg images:
 * a few images run the launch geometry of a large batch.  The two-group entry decides on the planning counts whether the
 * launch is merged (gcv_dw_plan2). */
int gcv_k_dwconv7_ln_planned(int dtype, const void* x, const float* wdw, const float* bdw, const float* lnw,
                             const float* lnb, void* y, int nimg, int H, int W, int C, float eps, int plan_nimg,
                             gcv_stream s);
int gcv_k_dwconv7_ln2_planned(int dtype, const void* x0, void* y0, int nimg0, int H0, int W0, const void* x1, void* y1,
                              int nimg1, int H1, int W1, const float* wdw, const float* bdw, const float* lnw,
                              const float* lnb, int C, float eps, int plan_nimg0, int plan_nimg1, gcv_stream s);
/* Test query: out1[0] = 1 if gcv_k_dwconv7_ln2 runs these two 16-byte aligned groups as one merged launch, 0 if as two.
 * No HIP call: works without a GPU. */
int gcv_dw_plan2(int dtype, int nimg0, int H0, int W0, int nimg1, int H1, int W1, int C, int* out1);
/* Test query: 1 if gcv_convnext_forward on a handle of backbone `arch` (GCV_CONVNEXT_TINY / _LARGE) runs resolution `res`,
 * 0 if it refuses it (the rule it applies itself).  No HIP call: works without a GPU. */
int gcv_convnext_res_ok(int arch, int res);
int gcv_k_ln_patchify(int dtype, const void* x, const float* w, const float* b, void* out, int nimg, int H, int W,
                      int C, float eps, gcv_stream s);
int gcv_k_layernorm_rows(int dtype, const void* x, const float* w, const float* b, void* out, int64_t rows, int C,
                         float eps, gcv_stream s);
int gcv_k_pool_ln(int dtype, const void* x, const float* w, const float* b, void* out, int nimg, int HW, int C,
                  float eps, gcv_stream s);
/* gcv_k_pool_ln with the row mapping the networks use: image b of the launch -> output row
 * (b % seg_n) * row_stride + row0 + b / seg_n (seg_n <= 0: plain order, as gcv_k_pool_ln) */
int gcv_k_pool_ln_rows(int dtype, const void* x, const float* w, const float* b, void* out, int nimg, int HW, int C,
                       float eps, int seg_n, int row_stride, int row0, gcv_stream s);
int gcv_k_conv3_first(int dtype, const void* x, int64_t sb, int64_t sc, int64_t sy, int64_t sx, const float* wp,
                      const float* bias, void* out, int nimg, int H, int W, int pool, int act, gcv_stream s);
int gcv_k_convt2_small(int dtype, const void* x, const float* wp, const float* bias, void* out, int nimg, int H,
                       int W, int act, gcv_stream s);
int gcv_k_reparam(int dtype, const float* partial, int splitk, const float* bias, const float* eps, float* mu_out,
                  void* z_nhwc, int B, int N, gcv_stream s);
int gcv_k_head_tail(int dtype, const void* h, const float* w, const float* bias, float* logits, int B, int K,
                    gcv_stream s);
/* The head as the networks run it (model/genconvit_ed.py:87, model/genconvit_vae.py:114: fc2(act(fc(.)))): the hidden layer's
 * split-K partials (splitk, B, K) fp32 are reduced on the way in, h = act(sum + b1) rounded to the storage dtype, then
 * logits = h . w^T + bias with w (2, K), in one kernel.  act: GCV_ACT_* code. */
int gcv_k_head_tail_splitk(int dtype, const float* partial, int splitk, const float* b1, int act, const float* w,
                           const float* bias, float* logits, int B, int K, gcv_stream s);
int gcv_k_resize_mse(int dtype, const void* xhat, const void* img, void* recon, float* msepart, float* mse, int B,
                     gcv_stream s);

/* Swin-T pieces (timm swin_tiny_patch4_window7_224): W-MSA / SW-MSA over 7x7
 * windows with relative-position bias + shift mask on a (B,H,W,3C) qkv tensor; PatchMerging's
 * 2x2 gather + LayerNorm(4C); mean over tokens. */
int gcv_k_swin_window_attn(int dtype, const void* qkv, const float* rpb, void* out, int nimg, int H, int W, int C,
                           int nH, int shift, gcv_stream s);
int gcv_k_patch_merge_ln(int dtype, const void* x, const float* w, const float* b, void* out, int nimg, int H, int W,
                         int C, float eps, gcv_stream s);
int gcv_k_mean_tokens(int dtype, const void* x, void* out, int nimg, int L, int C, gcv_stream s);

/* Grad-CAM backward kernels, one launch each (csrc/cam.h, csrc/cam_bwd.h; the chains are gcv_*_explain and gcv_*_explain_at).
 * Gradients are fp32 in every storage dtype; x, A, fc_w, bb_pre, w, and the `out` of scale_rows / `pre` of gelu_bwd are in the
 * storage dtype.  target, gamma and cam224 may be null.  Pass p's map of image b lands at cam + b * cam_ld + off_p; a launch with
 * npass = 1 ignores the second pass's arguments. */
int gcv_k_head_bwd(int dtype, const float* partial, int S, const float* b1, const float* fc2_w, const float* logits,
                   const int* target, const void* fc_w, const void* bb_pre, float* dfeat, int B, int act, gcv_stream s);
int gcv_k_bb_bwd(int dtype, const float* dfeat, const void* w, float* dpool, int rows, int C, gcv_stream s);
int gcv_k_cam(int dtype, int C, int npass, const void* A0, const void* A1, int side0, int side1, int off0, int off1,
              int cam_ld, int up_pass, const float* lnw, const float* dpool, float* cam, float* cam224, float eps, int B,
              gcv_stream s);
int gcv_k_pool_ln_bwd(int dtype, int C, int npass, const void* A0, const void* A1, int hw0, int hw1, int tok0_0,
                      int tok0_1, const float* lnw, const float* dpool, float* dA, float eps, int B, gcv_stream s);
int gcv_k_scale_rows(int dtype, const float* g, const float* gamma, void* out, float* inv, int M, int C, gcv_stream s);
int gcv_k_gelu_bwd(int dtype, const float* dh, const float* inv_in, void* pre, float* inv_out, int M, int C4,
                   gcv_stream s);
int gcv_k_dw_ln_bwd(int dtype, const void* x, const float* dw_w, const float* dw_b, const float* ln_w, const float* dxln,
                    const float* inv, float* ddw, int nimg, int side, int C, float eps, gcv_stream s);
int gcv_k_dw_dgrad_res(const float* ddw, const float* dw_w, float* g, int nimg, int side, int C, gcv_stream s);
int gcv_k_down_ln_bwd(int dtype, const void* x, const float* ln_w, const float* dP, const float* inv, float* dA2,
                      int nimg, int side2, int C2, float eps, gcv_stream s);
int gcv_k_cam2(int dtype, int C2, int npass, const void* A0, const void* A1, const float* dA0, const float* dA1,
               int side0, int side1, int off0, int off1, int cam_ld, int up_pass, float* cam, float* cam224, float* alpha,
               int B, gcv_stream s);

/* Fused ConvNeXt MLP for C = 96 / 192, 16-bit storage:
 * out = resid + gamma * (W2 . GELU(W1 . x + b1) + b2) with the 4C hidden activation kept on chip
 * (timm ConvNeXtBlock: mlp.fc1 -> GELU -> mlp.fc2 -> * gamma -> + shortcut).  w2_f32: (C,4C) fp32 device. */
int gcv_k_fused_mlp(int dtype, int C, const void* x, const void* w1, const float* b1, const float* w2_f32,
                    const float* b2, const float* gamma, const void* resid, void* out, int M, gcv_stream s);
/* The last block of ConvNeXt stage 0 / 1 as the network runs it: the MLP above with the stage boundary's
 * `downsample` LayerNorm2d + the 2x2 space-to-depth of its Conv2d(k=2, s=2) in the epilogue (timm ConvNeXtStage.downsample,
 * SURVEY A.1; call sites model/genconvit_ed.py:82-83, model/genconvit_vae.py:111-112).  Tokens [tok0[i], tok0[i+1]) (the
 * last segment ends at M) are whole images of hw[i] = H*W pixels, W = wd[i], H and W even; `out` receives the patch rows
 * (M/4, 4C), (dy, dx, c) innermost, segment i starting at row out0[i] = tok0[i] / 4; the (M, C) residual stream is not
 * written.  C = 96 (M >= 65536 tokens: the LDS-resident kernel) or C = 192; nseg <= 4; host int arrays. */
int gcv_k_fused_mlp_lnp(int dtype, int C, const void* x, const void* w1, const float* b1, const float* w2_f32,
                        const float* b2, const float* gamma, const void* resid, const float* ln_w, const float* ln_b,
                        float eps, int nseg, const int* tok0, const int* hw, const int* wd, const int* out0, void* out, int M,
                        gcv_stream s);
/* Test entries: the two launches above with the persistent kernels (C = 192; C = 96 at M >= 65536) held to at most wg_cap
 * workgroups, 1 ... 256; the networks run 256, one per CU.  A lower cap gives every workgroup more passes (C = 192) or
 * every wave more tiles (C = 96): a few thousand tokens run the pass count of a large batch.  The other kernels ignore it. */
int gcv_k_fused_mlp_planned(int dtype, int C, const void* x, const void* w1, const float* b1, const float* w2_f32,
                            const float* b2, const float* gamma, const void* resid, void* out, int M, int wg_cap,
                            gcv_stream s);
int gcv_k_fused_mlp_lnp_planned(int dtype, int C, const void* x, const void* w1, const float* b1, const float* w2_f32,
                                const float* b2, const float* gamma, const void* resid, const float* ln_w,
                                const float* ln_b, float eps, int nseg, const int* tok0, const int* hw, const int* wd,
                                const int* out0, void* out, int M, int wg_cap, gcv_stream s);
/* Test query: the kernels and grids of the ConvNeXt MLP at C channels and M tokens, persistent kernels held to wg_cap
 * workgroups (256: as the networks launch).  out8[0] = kind, the rest by kind:
 *   0 two tile GEMMs (fp32; 16-bit at other widths than below): zeros, see gcv_gemm_plan
 *   1 C = 96    {1 LDS-resident persistent kernel / 0 tile kernel, workgroups, 32-token wave tiles, most tiles per wave}
 *   2 C = 192   {256-token passes, workgroups, most passes per workgroup}
 *   3 C = 384   {256-token pw1 tiles, hidden ranges ns, 32-wide hidden chunks per workgroup, pw2 tile BN, its ring depth D,
 *                its 32-token blocks TB, pw2 workgroups}
 * No HIP call: works without a GPU. */
int gcv_mlp_plan(int dtype, int C, int M, int wg_cap, int* out8);
/* The same launch, timed: the weights are packed once, then `iters` launches of the MLP kernel(s) alone are bracketed by
 * HIP events on `s` (the call synchronises).  ms3[0] = average ms per MLP; for the C = 384 kernel pair ms3[1] / ms3[2] are
 * pw1+GELU / pw2+scale+residual timed separately, else 0.  Used by profiles/microbench.py; `out` may alias `resid`. */
int gcv_k_fused_mlp_timed(int dtype, int C, const void* x, const void* w1, const float* b1, const float* w2_f32,
                          const float* b2, const float* gamma, const void* resid, void* out, int M, int iters,
                          float* ms3, gcv_stream s);

#if defined(GCV_BUILD)
#pragma GCC visibility pop
#endif

#ifdef __cplusplus
}
#endif
#endif /* GENCONVIT_HIP_H */
