// Host-side driver of the GenConViT path: weight packing, workspace arena, per-launch
// profiler and the ED / VAE / ConvNeXt-T forward schedules (one instantiation per storage dtype).
#pragma once
#include <map>
#include <memory>
#include <functional>
#include <string>
#include <vector>

#include "common.h"

namespace gcv {

struct TensorRef {
  const float* data;
  int64_t numel;
  bool on_device;
};
typedef std::map<std::string, TensorRef> TensorMap;

// ---- per-launch profiler (HIP events on the launch stream) ------------------
struct ProfRecord {
  std::string tag;      // semantic op, e.g. "cnx.pw1", "cnx.dwconv_ln"
  double flops;         // algorithmic FLOPs of the launch (2*M*N*K for GEMMs)
  double bytes;         // algorithmic HBM bytes of the launch (unique reads + writes)
  hipEvent_t e0, e1;
};

// roctx ranges: while a handle's profiling is on, every tagged launch is also bracketed by a
// roctxRangePushA(tag) / roctxRangePop pair, so `rocprofv3 --marker-trace --kernel-trace` groups the kernels by the same
// semantic tags gcv_profile_report() uses.  The marker library is bound at run time (rocprofiler-sdk's roctx, then the legacy
// libroctx64) and only when profiling is switched on; without it the calls are no-ops.
void roctx_push(const char* tag);
void roctx_pop();

struct Profiler {
  bool enabled = false;
  std::vector<ProfRecord> recs;
  std::vector<hipEvent_t> pool;
  size_t next_event = 0;
  hipEvent_t get_event();
  void reset() { recs.clear(); next_event = 0; }
  ~Profiler();
};

// ---- test taps (gcv_tap_set, include/genconvit_hip.h) -------------------------
// A caller-owned device buffer that the forwards copy one named intermediate into.  A backbone tap covers every segment of
// the network's token stream; `mask` collects the segments whose copy was enqueued by the current forward and `need` is
// the set it takes to fill the buffer, so a tensor that some launch of the dispatch never stores reads as "not written".
struct Tap {
  void* dst = nullptr;
  size_t bytes = 0;
  unsigned mask = 0, need = 0;
};
bool tap_name_known(const std::string& name, int arch);

// ---- explain (gcv_*_explain, include/genconvit_hip.h) ---------------------------------------------------------------
// Grad-CAM request of one network's forward: target (B) device ints or null (argmax), maps at cam + b * cam_ld (the
// network's layout), cam224 (B, 224, 224) nullable.  layer: the ConvNeXt stage whose output the maps are taken at: 3 (the
// heads' backward alone, cam.h) or 2 (plus the backward of stage 3 and of the down-sampling in front of it, cam_bwd.h).
struct Explain {
  const int* target = nullptr;
  float* cam = nullptr;
  int cam_ld = 0;
  float* cam224 = nullptr;
  int layer = 3;
};

// ---- ConvNeXt backbone architecture (gcv_create_arch) ------------------------
// timm 0.6.5 convnext_tiny / convnext_large: same stem, block, downsample and head, widths and stage depths differ
struct CnxArch {
  int dims[4];
  int depths[4];
  int nblocks() const { return depths[0] + depths[1] + depths[2] + depths[3]; }
};
constexpr int kMaxCnxBlocks = 36;
inline const CnxArch& cnx_arch(int arch) {       // arch: GCV_CONVNEXT_TINY (0) / GCV_CONVNEXT_LARGE (1)
  static const CnxArch tiny{{96, 192, 384, 768}, {3, 3, 9, 3}}, large{{192, 384, 768, 1536}, {3, 3, 27, 3}};
  return arch == 1 ? large : tiny;
}
// The resolutions gcv_convnext_forward runs (gcv_convnext_res_ok): multiples of 4 in [32, 224] whose four maps all have a
// depthwise kernel (dw_select, dwconv_impl.h).  The maps are res / 4 pixels wide, halved with floor at each stage boundary:
// the stage-3 map is res / 32.  ConvNeXt-T has the generic tile kernel at every width; at ConvNeXt-L's C = 1536 there are
// kernels for maps up to 4 x 4 and for 7 x 7 only, so a 5- or 6-pixel stage-3 map (res 160 ... 220) is refused before
// anything is launched.
inline bool cnx_res_ok(int arch, int res) {
  if (res % 4 != 0 || res < 32 || res > 224) return false;
  const int s3 = res / 32;
  return arch != 1 || s3 <= 4 || s3 == 7;
}
inline const char* cnx_res_rule(int arch) {
  return arch == 1 ? "resolution must be a multiple of 4 in [32,156], or 224, on a ConvNeXt-L handle (no C = 1536 depthwise "
                     "kernel for the 5- and 6-pixel stage-3 maps of 160 ... 220)"
                   : "resolution must be a multiple of 4 in [32,224]";
}

// ---- abstract network (dtype erased) ----------------------------------------
struct NetBase {
  int device = 0;
  int dtype = 0;
  int max_batch = 0;
  int arch = 0;                   // GCV_CONVNEXT_TINY / GCV_CONVNEXT_LARGE: the backbone of both networks of the handle
  Profiler prof;
  bool in_ensemble = false;   // set by gcv_genconvit_forward around vae_forward: the VAE shares the GPU with the ED network
  // host-side enqueue order of the ensemble (gcv_genconvit_forward): called by vae_forward once its encoder -> mu ->
  // decoder chain is enqueued and before its backbone pass, to enqueue the ED network on its own stream in between
  std::function<int()> after_chain;
  std::map<std::string, Tap> taps;   // empty unless a test registered one: then no forward looks at it
  virtual ~NetBase() {}
  virtual int init() = 0;
  virtual int load_ed(const TensorMap& w) = 0;
  virtual int load_vae(const TensorMap& w) = 0;
  virtual int load_swin(const TensorMap& w, const std::string& prefix) = 0;
  virtual int ed_forward(const void* x, int B, float* logits, hipStream_t s) = 0;
  virtual int vae_forward(const void* x, const float* eps, int B, float* logits, void* recon224, float* mse,
                          float* kl, hipStream_t s) = 0;
  // the forwards above followed by the Grad-CAM chain (cam.h) on the same stream(s); the logits are the forward's
  virtual int ed_explain(const void* x, int B, float* logits, const Explain& ex, hipStream_t s) = 0;
  virtual int vae_explain(const void* x, const float* eps, int B, float* logits, const Explain& ex, hipStream_t s) = 0;
  virtual int convnext_forward(int which /*0 ed backbone, 1 vae backbone*/, const void* x, int B, int res,
                               void* logits1000, hipStream_t s) = 0;
  virtual int swin_forward(const void* x, int B, void* logits1000, hipStream_t s) = 0;
  virtual size_t workspace_bytes() const = 0;
};

NetBase* make_net_f32();
NetBase* make_net_f16();
NetBase* make_net_bf16();

}  // namespace gcv
