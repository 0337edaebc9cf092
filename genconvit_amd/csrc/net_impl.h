// NetImpl<T>: weight packing + forward schedules (included by net_{f32,f16,bf16}.hip).
//
// Data layout in HBM
//   activations : NHWC "token major" (tokens, C) in T; several images / passes that share a weight
//                 set are concatenated along the token axis so pointwise GEMMs run once over all of them
//   GEMM weights: (N, K) row-major in T (nn.Linear layout); conv weights re-ordered to K = (ky,kx,ci)
//   small params: fp32 (biases, LayerNorm affine, layer-scale gamma, depthwise taps [49][C])
//   workspace   : one arena sized by a dry run of both forwards at max_batch (no allocation per call)
#pragma once
#include <algorithm>
#include <cmath>
#include <cstdlib>
#include <cstring>

#include "cam.h"
#include "cam_bwd.h"
#include "cnx_mlp.h"
#include "gemm.h"
#include "kernels.h"
#include "net.h"
#include "swin.h"

namespace gcv {

// ---------------------------------------------------------------- host conversions
template <typename T> inline T host_cvt(float v);
template <> inline float host_cvt<float>(float v) { return v; }
template <> inline half_t host_cvt<half_t>(float v) { return (half_t)v; }
template <> inline bf16_t host_cvt<bf16_t>(float v) {
  uint32_t u;
  std::memcpy(&u, &v, 4);
  uint16_t h;
  if ((u & 0x7fffffffu) > 0x7f800000u) h = (uint16_t)((u >> 16) | 0x40);   // NaN stays NaN
  else h = (uint16_t)((u + 0x7fffu + ((u >> 16) & 1u)) >> 16);              // round to nearest even
  bf16_t r;
  std::memcpy(&r, &h, 2);
  return r;
}

// ---------------------------------------------------------------- device memory owners
struct WeightStore {
  std::vector<void*> ptrs;
  size_t bytes = 0;
  ~WeightStore() { clear(); }
  void clear() {
    for (void* p : ptrs) (void)hipFree(p);
    ptrs.clear();
    bytes = 0;
  }
  void* raw(size_t n) {
    void* p = nullptr;
    if (hipMalloc(&p, n ? n : 16) != hipSuccess) return nullptr;
    ptrs.push_back(p);
    bytes += n;
    return p;
  }
  template <typename U> U* upload(const std::vector<U>& h) {
    U* p = (U*)raw(h.size() * sizeof(U));
    if (!p) return nullptr;
    if (hipMemcpy(p, h.data(), h.size() * sizeof(U), hipMemcpyHostToDevice) != hipSuccess) return nullptr;
    return p;
  }
};

struct Arena {
  char* base = nullptr;
  size_t cap = 0, off = 0, peak = 0;
  bool dry = false;
  bool overflow = false;
  size_t mark() const { return off; }
  void release(size_t m) { off = m; }
  void* alloc(size_t bytes) {
    const size_t a = (off + 255) & ~(size_t)255;
    off = a + bytes;
    peak = std::max(peak, off);
    if (!dry && off > cap) { overflow = true; return base; }
    return base + a;
  }
  template <typename U> U* get(int64_t n) { return (U*)alloc((size_t)n * sizeof(U)); }
};
// releases an arena mark on every exit path of a forward (an error return included); `overflow` says that a live
// allocation reaches past the arena, so it ends with the scope that gives the arena back: a forward that was refused for
// its size leaves the handle as it found it
struct ArenaScope {
  Arena& a;
  const size_t m;
  explicit ArenaScope(Arena& a_) : a(a_), m(a_.mark()) {}
  ~ArenaScope() {
    a.release(m);
    if (a.off <= a.cap) a.overflow = false;
  }
};

// device-side permute+cast for the 25088x12544 mu/var matrices: columns c*196+hw -> hw*128+c so the
// NHWC encoder output (B,14,14,128) can be used as the GEMM A operand without a transpose.
template <typename T>
__global__ void __launch_bounds__(256) pack_mu_kernel(const float* __restrict__ src, T* __restrict__ dst, int64_t total) {
  const int64_t o = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (o >= total) return;
  const int64_t n = o / 25088;
  const int k = (int)(o - n * 25088);
  const int hw = k >> 7, c = k & 127;
  dst[o] = from_f<T>(src[n * 25088 + c * 196 + hw]);
}

// ---------------------------------------------------------------- packed weights
template <typename T> struct CnxBlockW {
  float *dw_w, *dw_b, *ln_w, *ln_b;
  CnxMlpW<T> mlp;
};
template <typename T> struct CnxW {
  float *stem_w, *stem_b, *stem_lnw, *stem_lnb;
  CnxBlockW<T> blk[kMaxCnxBlocks];
  struct { float *ln_w, *ln_b, *b; T* w; } down[3];
  float *head_lnw, *head_lnb, *head_fc_b;
  T* head_fc_w;
  // explain at stage 2 (cam_bwd.h): the transposes of stage 3's fc1 (C3, 4 C3) / fc2 (4 C3, C3) and of the stage 2 -> 3
  // down-sampling weight (4 C2, C3), so that dY . W runs through the (N, K)-row GEMMs
  T *bwd_w1t[3], *bwd_w2t[3], *bwd_downt;
};
template <typename T> struct HeadW {
  T* fc_w;        // (500, 2000)
  float* fc_b;
  float* fc2_w;   // [2][500]
  float* fc2_b;
};
template <typename T> struct EdW {
  float *enc1_w, *enc1_b;            // [27][16]
  T* enc_w[4];                       // layers 2..5 (Cout, 9*Cin)
  float* enc_b[4];
  T* dec_w[4];                       // layers 1..4 ((dy,dx,co), ci)
  float* dec_b[4];
  float *dec5_w, *dec5_b;            // [16][2][2][3]
  HeadW<T> head;
};
template <typename T> struct VaeW {
  float *enc1_w, *enc1_b;            // BN folded
  T* enc_w[3];
  float* enc_b[3];
  T *mu_w, *var_w;                   // (12544, 25088) K-permuted
  float *mu_b, *var_b;
  T* dec_w[3];
  float* dec_b[3];
  float *dec4_w, *dec4_b;
  HeadW<T> head;
};

// explain at stage 2: a segment's stage-2 output and the inputs of its stage-3 blocks, kept instead of overwritten
template <typename T> struct Stage3In {
  const T* s2 = nullptr;
  const T* x[3] = {nullptr, nullptr, nullptr};
};
template <typename T> struct Seg {
  const T* x;
  int64_t sb, sc, sy, sx;   // element strides of the (n,3,H,W) input view
  int n, H, W;
  T* out;                   // backbone logits (n,1000) written at out + i*out_ld
  int out_ld;
  int act;
  T* pre = nullptr;           // explain: the backbone logits before `act`, at pre + i*out_ld (else null)
  const T** s3 = nullptr;     // explain: receives this segment's stage-3 tokens (the pass then keeps its buffers)
  Stage3In<T>* in3 = nullptr; // explain at stage 2: receives what stage 3 read (its blocks then write a buffer each)
};

template <typename T> struct NetImpl : NetBase {
  WeightStore ws_ed, ws_vae, ws_swin;
  CnxW<T> bb_ed{}, bb_vae{};
  EdW<T> ed{};
  VaeW<T> vae{};
  SwinW<T> swin{};
  bool has_ed = false, has_vae = false, has_swin = false;
  Arena arena;
  hipStream_t cur = nullptr;
  // Schedule of vae_forward.  SPLIT: backbone(x) — which depends on nothing but the input — runs on a side stream while
  // the encoder / mu GEMM / decoder chain (small, latency-bound launches) and then backbone(x_hat) run on the caller's
  // stream.  MERGED: one stream, one two-segment backbone pass.  Alone on the GPU the split hides the codec chain
  // (vae B=32 bf16: 18.3k vs 15.2k frames/s); inside gcv_genconvit_forward the ED network already fills those gaps and
  // the merged pass wins (7.49 vs 7.58-7.62 ms per step in paired runs: the round-3 MLP kernels pay per 256-token pass
  // and prefer one launch over two smaller ones).  Default: split when called on its own, merged inside the ensemble;
  // GCV_VAE_SPLIT=0 / 1 forces one of them.  Both are under test (tests/test_parity_gpu.py, fresh_vae).
  int vae_split_env = [] { const char* e = std::getenv("GCV_VAE_SPLIT"); return e ? (std::atoi(e) != 0 ? 1 : 0) : -1; }();
  hipStream_t vae_side = nullptr;                      // (one per handle; the ED and the VAE network are separate handles)
  hipEvent_t vae_fork = nullptr, vae_join = nullptr;
  // the caller's stream waits for the side stream before the head reads its half of `feat` — and on every early return,
  // so that whatever was enqueued is ordered before the caller's next work
  struct Join {
    hipStream_t s = nullptr; hipEvent_t ev = nullptr;
    void arm(hipStream_t s_, hipEvent_t ev_) { s = s_; ev = ev_; }
    void now() { if (ev) { (void)hipStreamWaitEvent(s, ev, 0); ev = nullptr; } }
    ~Join() { now(); }
  };
  // (test taps) the segments of one network's backbone token stream in the library's concatenation order; a run_convnext call
  // covers segments [first, first + nseg of the call).
  struct TapPass {
    const char* net;      // "ed" / "vae"
    int nall, first;
    int n[4], H[4], W[4];
  };
  // run one backbone pass on the side stream, forked from `s` here
  int side_pass(const CnxW<T>& w, const Seg<T>* seg, hipStream_t s, Join& join, const TapPass* tp) {
    if (!arena.dry) {
      if (!vae_side) {
        GCV_CHECK_HIP(hipStreamCreateWithFlags(&vae_side, hipStreamNonBlocking));
        GCV_CHECK_HIP(hipEventCreateWithFlags(&vae_fork, hipEventDisableTiming));
        GCV_CHECK_HIP(hipEventCreateWithFlags(&vae_join, hipEventDisableTiming));
      }
      GCV_CHECK_HIP(hipEventRecord(vae_fork, s));
      GCV_CHECK_HIP(hipStreamWaitEvent(vae_side, vae_fork, 0));
      cur = vae_side;
    }
    const int rc = run_convnext(w, seg, 1, true, tp);
    cur = s;
    if (!arena.dry && hipEventRecord(vae_join, vae_side) == hipSuccess) join.arm(s, vae_join);
    return rc;
  }

  ~NetImpl() override {
    if (arena.base) (void)hipFree(arena.base);
    if (vae_side) (void)hipStreamDestroy(vae_side);
    if (vae_fork) (void)hipEventDestroy(vae_fork);
    if (vae_join) (void)hipEventDestroy(vae_join);
  }

  size_t workspace_bytes() const override { return arena.cap; }

  // ------------------------------------------------------------ launch plumbing
  template <class F> int run(const char* tag, double flops, double bytes, F&& f) {
    if (arena.dry) return 0;
    if (!prof.enabled) return f();
    ProfRecord r;
    r.tag = tag;
    r.flops = flops;
    r.bytes = bytes;
    r.e0 = prof.get_event();
    r.e1 = prof.get_event();
    roctx_push(tag);
    struct Pop { ~Pop() { roctx_pop(); } } pop;     // closes the range on every exit path
    GCV_CHECK_HIP(hipEventRecord(r.e0, cur));
    const int rc = f();
    GCV_CHECK_HIP(hipEventRecord(r.e1, cur));
    prof.recs.push_back(r);
    return rc;
  }

  int gemm(const char* tag, const GemmArgs& g, int a_mode, int epi) {
    const double flops = 2.0 * g.M * (double)g.N * g.K;
    double a_bytes = (a_mode == A_PLAIN) ? (double)g.M * g.K : (double)g.M * (1 << g.cin_log2);
    if (a_mode == A_IM2COL3_S2) a_bytes *= 4.0;     // input has 4x the pixels of the output
    double c_bytes = (double)g.M * g.N;
    if (epi == EPI_POOL4) c_bytes *= 0.25;
    if (epi == EPI_RESID) c_bytes *= 2.0;
    double bytes = sizeof(T) * (a_bytes + (double)g.N * g.K + c_bytes);
    if (epi == EPI_SPLITK) bytes = sizeof(T) * (a_bytes + (double)g.N * g.K) + 4.0 * g.splitk * (double)g.M * g.N;
    return run(tag, flops, bytes, [&] { return launch_gemm<T>(g, a_mode, epi, cur); });
  }

  // ------------------------------------------------------------ test taps (Tap in net.h, gcv_tap_set)
  // Nothing below runs unless a tap is registered: the forwards pass a null TapPass and skip every tap call when `taps` is
  // empty.  Copies are enqueued on `cur`, the stream that produced the tensor.
  void tap_reset(const char* net) {
    const size_t k = std::strlen(net);
    for (auto& kv : taps)
      if (kv.first.compare(0, k, net) == 0 && kv.first[k] == '.') kv.second.mask = kv.second.need = 0;
  }
  // `bytes` from `src` into tap `name` at byte offset `off`; `total`: the tap's size in this forward.  rows > 1: `rows`
  // rows of `bytes`, `spitch` bytes apart in the source, packed in the tap.  segbits / need: see Tap.
  int tap_copy(const std::string& name, size_t total, size_t off, const void* src, size_t bytes, unsigned segbits,
               unsigned need, size_t rows = 1, size_t spitch = 0) {
    auto it = taps.find(name);
    if (it == taps.end() || arena.dry) return 0;
    Tap& t = it->second;
    if (t.bytes != total) {
      set_error("tap '" + name + "': buffer of " + std::to_string(t.bytes) + " bytes, this forward stores " +
                std::to_string(total));
      return -8;
    }
    char* d = (char*)t.dst + off;
    if (rows == 1) GCV_CHECK_HIP(hipMemcpyAsync(d, src, bytes, hipMemcpyDeviceToDevice, cur));
    else GCV_CHECK_HIP(hipMemcpy2DAsync(d, bytes, src, spitch, bytes, rows, hipMemcpyDeviceToDevice, cur));
    t.mask |= segbits;
    t.need = need;
    return 0;
  }
  int tap_net(const char* name, const void* src, size_t bytes) { return tap_copy(name, bytes, 0, src, bytes, 1u, 1u); }
  // per-image elements of a backbone tap of segment s: kind 0 stem, 1 block output of stage i, 2 the operand of stage i's
  // downsample GEMM, 3 pooled rows
  int64_t tap_img_elems(const TapPass& tp, int s, int kind, int i) const {
    const int* dims = cnx_arch(arch).dims;
    const int64_t hw = (int64_t)((tp.H[s] / 4) >> i) * ((tp.W[s] / 4) >> i);
    return kind == 3 ? dims[3] : kind == 2 ? hw * 4 * dims[i - 1] : hw * dims[i];
  }
  // segments [tp.first, tp.first + nseg) of backbone tap `<net>.bb.<what>`, contiguous at `src` (pool_ld > 0: pooled rows
  // stored frame-major, row pool_ld * frame + segment)
  int tap_bb(const TapPass& tp, int nseg, const std::string& what, int kind, int i, const T* src, int pool_ld = 0) {
    const std::string name = std::string(tp.net) + ".bb." + what;
    if (!taps.count(name)) return 0;
    int64_t total = 0, off = 0, n = 0;
    for (int s = 0; s < tp.nall; ++s) {
      const int64_t e = tp.n[s] * tap_img_elems(tp, s, kind, i);
      if (s == tp.first) off = total;
      if (s >= tp.first && s < tp.first + nseg) n += e;
      total += e;
    }
    const unsigned need = (1u << tp.nall) - 1, bits = ((1u << nseg) - 1) << tp.first;
    if (!pool_ld) return tap_copy(name, total * sizeof(T), off * sizeof(T), src, n * sizeof(T), bits, need);
    const int C3 = cnx_arch(arch).dims[3];
    for (int s = 0; s < nseg; ++s) {
      GCV_TRY(tap_copy(name, total * sizeof(T), off * sizeof(T), src + s * C3, C3 * sizeof(T), bits, need,
                       tp.n[tp.first + s], (size_t)pool_ld * C3 * sizeof(T)));
      off += (int64_t)tp.n[tp.first + s] * C3;
    }
    return 0;
  }

  // ------------------------------------------------------------ weight fetch helpers
  static int fetch(const TensorMap& w, const std::string& name, int64_t numel, std::vector<float>& out) {
    auto it = w.find(name);
    if (it == w.end()) { set_error("missing weight tensor '" + name + "'"); return -4; }
    if (it->second.numel != numel) {
      set_error("weight tensor '" + name + "' has " + std::to_string(it->second.numel) + " elements, expected " +
                std::to_string(numel));
      return -4;
    }
    out.resize((size_t)numel);
    if (it->second.on_device) GCV_CHECK_HIP(hipMemcpy(out.data(), it->second.data, numel * 4, hipMemcpyDeviceToHost));
    else std::memcpy(out.data(), it->second.data, (size_t)numel * 4);
    return 0;
  }
  static std::vector<T> cast_vec(const std::vector<float>& v) {
    std::vector<T> o(v.size());
    for (size_t i = 0; i < v.size(); ++i) o[i] = host_cvt<T>(v[i]);
    return o;
  }

  int up_f32(const TensorMap& w, const std::string& name, int64_t n, WeightStore& st, float*& dst) {
    std::vector<float> v;
    GCV_TRY(fetch(w, name, n, v));
    GCV_UP(dst, st, v);
    return 0;
  }
  int up_cast(const TensorMap& w, const std::string& name, int64_t n, WeightStore& st, T*& dst) {
    std::vector<float> v;
    GCV_TRY(fetch(w, name, n, v));
    std::vector<T> c = cast_vec(v);
    GCV_UP(dst, st, c);
    return 0;
  }
  // nn.Linear weight (rows, cols) -> its transpose (cols, rows) in T
  int up_cast_t(const TensorMap& w, const std::string& name, int rows, int cols, WeightStore& st, T*& dst) {
    std::vector<float> v;
    GCV_TRY(fetch(w, name, (int64_t)rows * cols, v));
    std::vector<T> o((size_t)rows * cols);
    for (int r = 0; r < rows; ++r)
      for (int c = 0; c < cols; ++c) o[(size_t)c * rows + r] = host_cvt<T>(v[(size_t)r * cols + c]);
    GCV_UP(dst, st, o);
    return 0;
  }
  // Conv2d weight (Cout,Cin,2,2) -> ((ky,kx,ci), Cout) in T: the transpose of up_conv_gemm's pack
  int up_conv_gemm_t(const TensorMap& w, const std::string& name, int cout, int cin, WeightStore& st, T*& dst) {
    std::vector<float> v;
    GCV_TRY(fetch(w, name, (int64_t)cout * cin * 4, v));
    std::vector<T> o((size_t)cout * cin * 4);
    for (int co = 0; co < cout; ++co)
      for (int ci = 0; ci < cin; ++ci)
        for (int q = 0; q < 4; ++q) o[((size_t)q * cin + ci) * cout + co] = host_cvt<T>(v[((size_t)co * cin + ci) * 4 + q]);
    GCV_UP(dst, st, o);
    return 0;
  }
  // Conv2d weight (Cout,Cin,kh,kw) [* per-Cout scale] -> (Cout, (ky,kx,ci)) in T
  int up_conv_gemm(const TensorMap& w, const std::string& name, int cout, int cin, int kh, int kw,
                   const std::vector<float>* scale, WeightStore& st, T*& dst) {
    std::vector<float> v;
    GCV_TRY(fetch(w, name, (int64_t)cout * cin * kh * kw, v));
    std::vector<T> o((size_t)cout * cin * kh * kw);
    for (int co = 0; co < cout; ++co)
      for (int ci = 0; ci < cin; ++ci)
        for (int ky = 0; ky < kh; ++ky)
          for (int kx = 0; kx < kw; ++kx) {
            float x = v[(((size_t)co * cin + ci) * kh + ky) * kw + kx];
            if (scale) x *= (*scale)[co];
            o[(size_t)co * cin * kh * kw + ((size_t)(ky * kw + kx)) * cin + ci] = host_cvt<T>(x);
          }
    GCV_UP(dst, st, o);
    return 0;
  }
  // ConvTranspose2d weight (Cin,Cout,2,2) -> ((dy,dx,co), ci) in T
  int up_convt_gemm(const TensorMap& w, const std::string& name, int cin, int cout, WeightStore& st, T*& dst) {
    std::vector<float> v;
    GCV_TRY(fetch(w, name, (int64_t)cin * cout * 4, v));
    std::vector<T> o((size_t)cin * cout * 4);
    for (int ci = 0; ci < cin; ++ci)
      for (int co = 0; co < cout; ++co)
        for (int dy = 0; dy < 2; ++dy)
          for (int dx = 0; dx < 2; ++dx)
            o[((size_t)(dy * 2 + dx) * cout + co) * cin + ci] = host_cvt<T>(v[(((size_t)ci * cout + co) * 2 + dy) * 2 + dx]);
    GCV_UP(dst, st, o);
    return 0;
  }
  // ConvTranspose2d weight (16,3,2,2) -> [ci][dy][dx][co] fp32
  int up_convt_small(const TensorMap& w, const std::string& name, WeightStore& st, float*& dst) {
    std::vector<float> v;
    GCV_TRY(fetch(w, name, 16 * 3 * 4, v));
    std::vector<float> o(16 * 12);
    for (int ci = 0; ci < 16; ++ci)
      for (int co = 0; co < 3; ++co)
        for (int dy = 0; dy < 2; ++dy)
          for (int dx = 0; dx < 2; ++dx) o[ci * 12 + (dy * 2 + dx) * 3 + co] = v[((ci * 3 + co) * 2 + dy) * 2 + dx];
    GCV_UP(dst, st, o);
    return 0;
  }
  // first conv (16,3,3,3) [* scale] -> [27][16] fp32, k = (ky*3+kx)*3 + ci
  int up_conv_first(const TensorMap& w, const std::string& name, const std::vector<float>* scale, WeightStore& st,
                    float*& dst) {
    std::vector<float> v;
    GCV_TRY(fetch(w, name, 16 * 27, v));
    std::vector<float> o(27 * 16);
    for (int co = 0; co < 16; ++co)
      for (int ci = 0; ci < 3; ++ci)
        for (int ky = 0; ky < 3; ++ky)
          for (int kx = 0; kx < 3; ++kx)
            o[((ky * 3 + kx) * 3 + ci) * 16 + co] = v[((co * 3 + ci) * 3 + ky) * 3 + kx] * (scale ? (*scale)[co] : 1.0f);
    GCV_UP(dst, st, o);
    return 0;
  }

  // packs a ConvNeXt block's MLP for its kind (cnx_mlp.h); the kinds that pack fc2 from fp32 get it uploaded here, for as
  // long as their packing kernels run
  int pack_mlp(const TensorMap& w, const std::string& fc2_name, int C, WeightStore& st, CnxMlpW<T>& mw) {
    if (mw.kind == MlpKind::Gemm) return 0;
    struct DevBuf {                        // freed on every exit path
      float* p = nullptr;
      ~DevBuf() { if (p) (void)hipFree(p); }
    } w2f;
    if (mlp_packs_from_f32(mw.kind)) {
      std::vector<float> v;
      GCV_TRY(fetch(w, fc2_name, (int64_t)4 * C * C, v));
      GCV_CHECK_HIP(hipMalloc((void**)&w2f.p, v.size() * 4));
      GCV_CHECK_HIP(hipMemcpy(w2f.p, v.data(), v.size() * 4, hipMemcpyHostToDevice));
    }
    GCV_TRY(pack_cnx_mlp<T>(mw, C, w2f.p, [&](size_t n) { return st.raw(n); }, nullptr));
    GCV_CHECK_HIP(hipDeviceSynchronize());
    return 0;
  }

  // the backbone of this handle's arch (cnx_arch): stages.{i}.blocks.{j} for j < depths[i], widths dims[i]
  int pack_convnext(const TensorMap& w, const std::string& p, WeightStore& st, CnxW<T>& o) {
    const CnxArch& A = cnx_arch(arch);
    const int C0 = A.dims[0], C3 = A.dims[3];
    {
      std::vector<float> v, t((size_t)48 * C0);
      GCV_TRY(fetch(w, p + "stem.0.weight", (int64_t)C0 * 48, v));
      for (int co = 0; co < C0; ++co)
        for (int k = 0; k < 48; ++k) t[k * C0 + co] = v[co * 48 + k];
      GCV_UP(o.stem_w, st, t);
    }
    GCV_TRY(up_f32(w, p + "stem.0.bias", C0, st, o.stem_b));
    GCV_TRY(up_f32(w, p + "stem.1.weight", C0, st, o.stem_lnw));
    GCV_TRY(up_f32(w, p + "stem.1.bias", C0, st, o.stem_lnb));
    int bi = 0;
    for (int i = 0; i < 4; ++i) {
      const int C = A.dims[i];
      if (i > 0) {
        const int Cp = A.dims[i - 1];
        const std::string d = p + "stages." + std::to_string(i) + ".downsample.";
        GCV_TRY(up_f32(w, d + "0.weight", Cp, st, o.down[i - 1].ln_w));
        GCV_TRY(up_f32(w, d + "0.bias", Cp, st, o.down[i - 1].ln_b));
        GCV_TRY(up_conv_gemm(w, d + "1.weight", C, Cp, 2, 2, nullptr, st, o.down[i - 1].w));
        GCV_TRY(up_f32(w, d + "1.bias", C, st, o.down[i - 1].b));
        if (i == 3) GCV_TRY(up_conv_gemm_t(w, d + "1.weight", C, Cp, st, o.bwd_downt));
      }
      for (int j = 0; j < A.depths[i]; ++j, ++bi) {
        const std::string b = p + "stages." + std::to_string(i) + ".blocks." + std::to_string(j) + ".";
        CnxBlockW<T>& k = o.blk[bi];
        {
          std::vector<float> v, t((size_t)49 * C);
          GCV_TRY(fetch(w, b + "conv_dw.weight", (int64_t)C * 49, v));
          for (int c = 0; c < C; ++c)
            for (int q = 0; q < 49; ++q) t[(size_t)q * C + c] = v[(size_t)c * 49 + q];
          GCV_UP(k.dw_w, st, t);
        }
        GCV_TRY(up_f32(w, b + "conv_dw.bias", C, st, k.dw_b));
        GCV_TRY(up_f32(w, b + "norm.weight", C, st, k.ln_w));
        GCV_TRY(up_f32(w, b + "norm.bias", C, st, k.ln_b));
        T *w1, *w2;
        float *b1, *b2, *gamma;
        GCV_TRY(up_cast(w, b + "mlp.fc1.weight", (int64_t)4 * C * C, st, w1));
        GCV_TRY(up_f32(w, b + "mlp.fc1.bias", 4 * C, st, b1));
        GCV_TRY(up_cast(w, b + "mlp.fc2.weight", (int64_t)4 * C * C, st, w2));
        GCV_TRY(up_f32(w, b + "mlp.fc2.bias", C, st, b2));
        GCV_TRY(up_f32(w, b + "gamma", C, st, gamma));
        k.mlp = CnxMlpW<T>{mlp_kind(sizeof(T), C), w1, w2, b1, b2, gamma};
        GCV_TRY(pack_mlp(w, b + "mlp.fc2.weight", C, st, k.mlp));
        if (i == 3) {
          GCV_REQUIRE(j < 3, "stage 3 has at most 3 blocks");
          GCV_TRY(up_cast_t(w, b + "mlp.fc1.weight", 4 * C, C, st, o.bwd_w1t[j]));
          GCV_TRY(up_cast_t(w, b + "mlp.fc2.weight", C, 4 * C, st, o.bwd_w2t[j]));
        }
      }
    }
    GCV_TRY(up_f32(w, p + "head.norm.weight", C3, st, o.head_lnw));
    GCV_TRY(up_f32(w, p + "head.norm.bias", C3, st, o.head_lnb));
    GCV_TRY(up_cast(w, p + "head.fc.weight", (int64_t)1000 * C3, st, o.head_fc_w));
    GCV_TRY(up_f32(w, p + "head.fc.bias", 1000, st, o.head_fc_b));
    return 0;
  }

  int pack_head(const TensorMap& w, WeightStore& st, HeadW<T>& h) {
    GCV_TRY(up_cast(w, "fc.weight", 500 * 2000, st, h.fc_w));
    GCV_TRY(up_f32(w, "fc.bias", 500, st, h.fc_b));
    GCV_TRY(up_f32(w, "fc2.weight", 2 * 500, st, h.fc2_w));
    GCV_TRY(up_f32(w, "fc2.bias", 2, st, h.fc2_b));
    return 0;
  }

  int load_ed(const TensorMap& w) override {
    GCV_CHECK_HIP(hipSetDevice(device));
    has_ed = false;
    ws_ed.clear();
    GCV_TRY(up_conv_first(w, "encoder.features.0.weight", nullptr, ws_ed, ed.enc1_w));
    GCV_TRY(up_f32(w, "encoder.features.0.bias", 16, ws_ed, ed.enc1_b));
    const int ech[5] = {16, 32, 64, 128, 256};
    const int eidx[4] = {3, 6, 9, 12};
    for (int l = 0; l < 4; ++l) {
      const std::string n = "encoder.features." + std::to_string(eidx[l]);
      GCV_TRY(up_conv_gemm(w, n + ".weight", ech[l + 1], ech[l], 3, 3, nullptr, ws_ed, ed.enc_w[l]));
      GCV_TRY(up_f32(w, n + ".bias", ech[l + 1], ws_ed, ed.enc_b[l]));
    }
    const int dch[5] = {256, 128, 64, 32, 16};
    const int didx[4] = {0, 2, 4, 6};
    for (int l = 0; l < 4; ++l) {
      const std::string n = "decoder.features." + std::to_string(didx[l]);
      GCV_TRY(up_convt_gemm(w, n + ".weight", dch[l], dch[l + 1], ws_ed, ed.dec_w[l]));
      GCV_TRY(up_f32(w, n + ".bias", dch[l + 1], ws_ed, ed.dec_b[l]));
    }
    GCV_TRY(up_convt_small(w, "decoder.features.8.weight", ws_ed, ed.dec5_w));
    GCV_TRY(up_f32(w, "decoder.features.8.bias", 3, ws_ed, ed.dec5_b));
    GCV_TRY(pack_convnext(w, "backbone.", ws_ed, bb_ed));
    GCV_TRY(pack_head(w, ws_ed, ed.head));
    has_ed = true;
    return 0;
  }

  int pack_mu(const TensorMap& w, const std::string& name, T*& dst) {
    auto it = w.find(name);
    const int64_t total = (int64_t)12544 * 25088;
    if (it == w.end() || it->second.numel != total) { set_error("missing or mis-sized '" + name + "'"); return -4; }
    dst = (T*)ws_vae.raw((size_t)total * sizeof(T));
    if (!dst) { set_error("hipMalloc failed for " + name); return -5; }
    const float* src = it->second.data;
    if (it->second.on_device) {
      hipLaunchKernelGGL((pack_mu_kernel<T>), dim3((unsigned)cdiv64(total, 256)), dim3(256), 0, 0, src, dst, total);
      GCV_CHECK_HIP(hipGetLastError());
      GCV_CHECK_HIP(hipDeviceSynchronize());
      return 0;
    }
    // host source (the published 2.6 GB VAE checkpoint, model/genconvit.py:16-21): streamed through a 49 MB staging
    // buffer, 512 rows at a time (the permutation stays inside a row), so the device never holds an fp32 copy
    constexpr int64_t kRows = 512;
    struct DevBuf {
      float* p = nullptr;
      ~DevBuf() { if (p) (void)hipFree(p); }
    } tmp;
    GCV_CHECK_HIP(hipMalloc((void**)&tmp.p, (size_t)(kRows * 25088 * 4)));
    for (int64_t r0 = 0; r0 < 12544; r0 += kRows) {
      const int64_t rows = std::min<int64_t>(kRows, 12544 - r0), n = rows * 25088;
      GCV_CHECK_HIP(hipMemcpy(tmp.p, src + r0 * 25088, (size_t)n * 4, hipMemcpyHostToDevice));
      hipLaunchKernelGGL((pack_mu_kernel<T>), dim3((unsigned)cdiv64(n, 256)), dim3(256), 0, 0, tmp.p, dst + r0 * 25088, n);
      GCV_CHECK_HIP(hipGetLastError());
      GCV_CHECK_HIP(hipDeviceSynchronize());
    }
    return 0;
  }

  int load_vae(const TensorMap& w) override {
    GCV_CHECK_HIP(hipSetDevice(device));
    has_vae = false;
    ws_vae.clear();
    const int ech[5] = {3, 16, 32, 64, 128};
    const int eidx[4] = {0, 3, 6, 9};
    for (int l = 0; l < 4; ++l) {
      const int c = ech[l + 1];
      const std::string cn = "encoder.features." + std::to_string(eidx[l]);
      const std::string bn = "encoder.features." + std::to_string(eidx[l] + 1);
      std::vector<float> cb, g, be, rm, rv;
      GCV_TRY(fetch(w, cn + ".bias", c, cb));
      GCV_TRY(fetch(w, bn + ".weight", c, g));
      GCV_TRY(fetch(w, bn + ".bias", c, be));
      GCV_TRY(fetch(w, bn + ".running_mean", c, rm));
      GCV_TRY(fetch(w, bn + ".running_var", c, rv));
      // eval-mode BatchNorm2d (eps 1e-5) folded into the conv: y = conv(x)*s + (b - mean)*s + beta
      std::vector<float> scale(c), bias(c);
      for (int i = 0; i < c; ++i) {
        scale[i] = g[i] / std::sqrt(rv[i] + 1e-5f);
        bias[i] = (cb[i] - rm[i]) * scale[i] + be[i];
      }
      if (l == 0) {
        GCV_TRY(up_conv_first(w, cn + ".weight", &scale, ws_vae, vae.enc1_w));
        GCV_UP(vae.enc1_b, ws_vae, bias);
      } else {
        GCV_TRY(up_conv_gemm(w, cn + ".weight", c, ech[l], 3, 3, &scale, ws_vae, vae.enc_w[l - 1]));
        GCV_UP(vae.enc_b[l - 1], ws_vae, bias);
      }
    }
    GCV_TRY(pack_mu(w, "encoder.mu.weight", vae.mu_w));
    GCV_TRY(up_f32(w, "encoder.mu.bias", 12544, ws_vae, vae.mu_b));
    vae.var_w = nullptr;
    vae.var_b = nullptr;
    if (w.count("encoder.var.weight")) {     // only needed for the optional KL output
      GCV_TRY(pack_mu(w, "encoder.var.weight", vae.var_w));
      GCV_TRY(up_f32(w, "encoder.var.bias", 12544, ws_vae, vae.var_b));
    }
    const int dch[4] = {256, 64, 32, 16};
    const int didx[3] = {0, 2, 4};
    for (int l = 0; l < 3; ++l) {
      const std::string n = "decoder.features." + std::to_string(didx[l]);
      GCV_TRY(up_convt_gemm(w, n + ".weight", dch[l], dch[l + 1], ws_vae, vae.dec_w[l]));
      GCV_TRY(up_f32(w, n + ".bias", dch[l + 1], ws_vae, vae.dec_b[l]));
    }
    GCV_TRY(up_convt_small(w, "decoder.features.6.weight", ws_vae, vae.dec4_w));
    GCV_TRY(up_f32(w, "decoder.features.6.bias", 3, ws_vae, vae.dec4_b));
    GCV_TRY(pack_convnext(w, "convnext_backbone.", ws_vae, bb_vae));
    GCV_TRY(pack_head(w, ws_vae, vae.head));
    has_vae = true;
    return 0;
  }

  int load_swin(const TensorMap& w, const std::string& prefix) override {
    GCV_CHECK_HIP(hipSetDevice(device));
    has_swin = false;
    ws_swin.clear();
    GCV_TRY((pack_swin<T>(*this, w, prefix, swin)));
    has_swin = true;
    return 0;
  }

  // ------------------------------------------------------------ ConvNeXt-T / -L (the handle's arch) over token segments
  // keep = true leaves the token buffers allocated (the caller releases its own mark): two passes of one forward that run
  // on different streams must not share them
  // tp: taps of this pass (null: none registered)
  int run_convnext(const CnxW<T>& w, const Seg<T>* segs, int nseg, bool keep = false, const TapPass* tp = nullptr) {
    int segn[4], h[4], wd[4];
    int64_t m[4], moff[4], M = 0;
    int ntot = 0;
    GCV_REQUIRE(nseg >= 1 && nseg <= 4, "1..4 segments");
    for (int s = 0; s < nseg; ++s) {
      GCV_REQUIRE(segs[s].H % 4 == 0 && segs[s].W % 4 == 0 && segs[s].n > 0, "segment geometry");
      segn[s] = segs[s].n;
      h[s] = segs[s].H / 4;
      wd[s] = segs[s].W / 4;
      m[s] = (int64_t)segs[s].n * h[s] * wd[s];
      moff[s] = M;
      M += m[s];
      ntot += segs[s].n;
    }
    const CnxArch& A = cnx_arch(arch);
    const int C0 = A.dims[0], C3 = A.dims[3];
    // the widest GEMM operand is stage 0's (M, 4 C0) hidden tensor (and every later stage's is smaller)
    GCV_REQUIRE(M * 4 * C0 < (int64_t)1 << 31, "token count too large for 32-bit GEMM indexing");
    bool saving = false, save3 = false;
    for (int s = 0; s < nseg; ++s) { saving = saving || segs[s].s3; save3 = save3 || segs[s].in3; }
    for (int s = 0; s < nseg; ++s) GCV_REQUIRE(!save3 || (segs[s].in3 && segs[s].s3), "stage-3 inputs are kept for every segment or none");
    GCV_REQUIRE(!save3 || A.depths[3] == 3, "stage 3 of three blocks");
    const size_t mk = arena.mark();
    T* X = arena.get<T>(M * C0);
    T* Y = arena.get<T>(M * C0);
    T* Hd = arena.get<T>(M * 4 * C0);
    T* Pool = arena.get<T>((int64_t)ntot * C3);
    // explain at stage 2: the down-sampling GEMM and each stage-3 block write a buffer of their own, so that the stage-2
    // output and every block's input outlive the pass (same kernels, same operands: only the output pointers differ)
    T* X3[4] = {nullptr, nullptr, nullptr, nullptr};
    if (save3) {
      int64_t M3 = 0;
      for (int s = 0; s < nseg; ++s) M3 += (int64_t)segs[s].n * (h[s] / 8) * (wd[s] / 8);
      for (int j = 0; j < 4; ++j) X3[j] = arena.get<T>(M3 * C3);
    }
    if (!arena.dry && arena.overflow) { set_error("workspace arena too small: batch exceeds max_batch"); return -6; }
    T* Xc = X;                    // the residual stream

    for (int s = 0; s < nseg; ++s) {
      const Seg<T>& g = segs[s];
      GCV_TRY(run("cnx.stem_ln", 2.0 * m[s] * C0 * 48, sizeof(T) * (double)m[s] * (48 + C0), [&] {
        return launch_stem_ln<T>(g.x, g.sb, g.sc, g.sy, g.sx, w.stem_w, w.stem_b, w.stem_lnw, w.stem_lnb,
                                 X + moff[s] * C0, g.n, h[s], wd[s], 1e-6f, cur, C0);
      }));
    }
    if (tp) GCV_TRY(tap_bb(*tp, nseg, "stem", 0, 0, X));
    int bi = 0;
    bool lnp_fused = false;       // the previous stage's last MLP has already written the LayerNorm'ed patches (into Hd)
    for (int i = 0; i < 4; ++i) {
      const int C = A.dims[i];
      if (i > 0) {
        const int Cp = A.dims[i - 1];
        int64_t newM = 0, noff[4];
        for (int s = 0; s < nseg;) {
          // neighbouring segments of one geometry (ED: reconstruction + original pass) are contiguous on both sides:
          // one launch over all their images, as for the depthwise kernel below
          int e = s, nimg = 0;
          int64_t mm = 0;
          const int64_t noff0 = newM;
          while (e < nseg && h[e] == h[s] && wd[e] == wd[s]) {
            noff[e] = newM;
            GCV_REQUIRE(h[e] / 2 > 0 && wd[e] / 2 > 0, "image too small for ConvNeXt downsampling");
            newM += (int64_t)segs[e].n * (h[e] / 2) * (wd[e] / 2);
            nimg += segs[e].n; mm += m[e]; ++e;
          }
          if (!lnp_fused)
            GCV_TRY(run("cnx.ln_patchify", 8.0 * mm * Cp, 2.0 * sizeof(T) * (double)mm * Cp, [&] {
              return launch_ln_patchify<T>(X + moff[s] * Cp, w.down[i - 1].ln_w, w.down[i - 1].ln_b,
                                           Y + noff0 * 4 * Cp, nimg, h[s], wd[s], Cp, 1e-6f, cur);
            }));
          s = e;
        }
        if (save3 && i == 3)
          for (int s = 0; s < nseg; ++s) segs[s].in3->s2 = X + moff[s] * Cp;
        for (int s = 0; s < nseg; ++s) {
          h[s] /= 2;
          wd[s] /= 2;
          m[s] = (int64_t)segs[s].n * h[s] * wd[s];
          moff[s] = noff[s];
        }
        M = newM;
        GemmArgs g{};
        if (save3 && i == 3) Xc = X3[0];
        g.A = lnp_fused ? Hd : Y; g.lda = 4 * Cp; g.Wt = w.down[i - 1].w; g.C = Xc; g.ldc = C; g.bias = w.down[i - 1].b;
        lnp_fused = false;
        g.M = (int)M; g.N = C; g.K = 4 * Cp; g.act = ACT_NONE; g.splitk = 1;
        if (tp) GCV_TRY(tap_bb(*tp, nseg, "s" + std::to_string(i) + ".down_in", 2, i, (const T*)g.A));
        GCV_TRY(gemm("cnx.down_gemm", g, A_PLAIN, EPI_BIAS_ACT));
      }
      // the residual stream after block j, unless its epilogue went straight to the stage boundary (lnp_fused)
      auto tap_block = [&](int j) {
        return tp && !lnp_fused ? tap_bb(*tp, nseg, "s" + std::to_string(i) + ".b" + std::to_string(j), 1, i, Xc) : 0;
      };
      for (int j = 0; j < A.depths[i]; ++j, ++bi) {
        const CnxBlockW<T>& k = w.blk[bi];
        T* Xn = Xc;               // the block's output: in place, unless its input is kept
        if (save3 && i == 3) {
          for (int s = 0; s < nseg; ++s) segs[s].in3->x[j] = Xc + moff[s] * C;
          Xn = X3[j + 1];
        }
        // neighbouring segments of one geometry (ED: reconstruction + original pass) are contiguous in the token
        // buffer: one launch over all their images (256 images fill the 256 CUs with whole-image row bands)
        int gs[4], gn[4], ng = 0;                        // geometry groups: first segment, images, tokens
        int64_t gm[4];
        for (int s = 0; s < nseg; ++ng) {
          GCV_REQUIRE(ng < 4, "at most four segments");
          int e = s + 1;
          gs[ng] = s; gn[ng] = segs[s].n; gm[ng] = m[s];
          while (e < nseg && h[e] == h[s] && wd[e] == wd[s]) { gn[ng] += segs[e].n; gm[ng] += m[e]; ++e; }
          s = e;
        }
        auto dw_bytes = [&](int q) { return 2.0 * sizeof(T) * (double)gm[q] * C + 49.0 * C * 4; };
        const T* gx[2] = {Xc + moff[gs[0]] * C, Xc + moff[gs[ng - 1]] * C};
        T* gy[2] = {Y + moff[gs[0]] * C, Y + moff[gs[ng - 1]] * C};
        // two groups (VAE: the 224- and the 112-pixel segment) whose kernels have a merged form share one grid: the small
        // group's workgroups follow the large one's without a launch boundary (dwconv_impl.h, launch_dwconv7_ln2)
        const bool al2 = ((reinterpret_cast<uintptr_t>(gx[0]) | reinterpret_cast<uintptr_t>(gx[1]) |
                           reinterpret_cast<uintptr_t>(gy[0]) | reinterpret_cast<uintptr_t>(gy[1])) & 15u) == 0;
        if (ng == 2 && dw_two_merged<T>(gn[0], h[gs[0]], wd[gs[0]], gn[1], h[gs[1]], wd[gs[1]], C, al2)) {
          GCV_TRY(run("cnx.dwconv7_ln", 2.0 * 49 * (gm[0] + gm[1]) * C, dw_bytes(0) + dw_bytes(1), [&] {
            return launch_dwconv7_ln2<T>(gx[0], gy[0], gn[0], h[gs[0]], wd[gs[0]], gx[1], gy[1], gn[1], h[gs[1]], wd[gs[1]],
                                         k.dw_w, k.dw_b, k.ln_w, k.ln_b, C, 1e-6f, cur);
          }));
        } else {
          for (int q = 0; q < ng; ++q) {
            const int s = gs[q];
            GCV_TRY(run("cnx.dwconv7_ln", 2.0 * 49 * gm[q] * C, dw_bytes(q), [&] {
              return launch_dwconv7_ln<T>(Xc + moff[s] * C, k.dw_w, k.dw_b, k.ln_w, k.ln_b, Y + moff[s] * C, gn[q], h[s],
                                          wd[s], C, 1e-6f, cur);
            }));
          }
        }
        // the last block of stages 0..2 may apply the stage boundary's LayerNorm2d + space-to-depth in its epilogue and write
        // the down-sampling GEMM's operand (into Hd: Y is still being read as x_ln); the residual stream then ends there
        LnpArgs l;
        const bool fuse = j == A.depths[i] - 1 && i < 3 && lnp_plan(l, k.mlp.kind, C, M, nseg, segn, h, wd);
        if (fuse) { l.w = w.down[i].ln_w; l.b = w.down[i].ln_b; l.eps = 1e-6f; }
        GCV_TRY(launch_cnx_mlp<T>(*this, k.mlp, C, Y, Xc, fuse ? Hd : Xn, Hd, (int)M, fuse ? &l : nullptr, cur));
        Xc = Xn;
        lnp_fused = fuse;
        GCV_TRY(tap_block(j));
      }
    }
    // pooling + LayerNorm: one launch over neighbouring segments of one map size (their tokens are contiguous).  When the
    // passes are the column blocks of one feature matrix (ED, VAE: equal frame counts, out = base + 1000 s, one leading
    // dimension, one activation) the pooled rows are written frame-major — row nseg * frame + pass — so that ONE classifier
    // GEMM over all nseg * n rows with ldc = 1000 writes the (n, nseg * 1000) matrix (round 4; one launch per pass before)
    bool one_fc = nseg > 1;
    for (int s = 1; s < nseg && one_fc; ++s)
      one_fc = segs[s].n == segs[0].n && segs[s].out == segs[0].out + 1000 * s && segs[s].out_ld == 1000 * nseg &&
               segs[0].out_ld == 1000 * nseg && segs[s].act == segs[0].act;
    int no = 0;
    for (int s = 0; s < nseg; ++s) {
      if (s == 0 || h[s] * wd[s] != h[s - 1] * wd[s - 1]) {
        int e = s, nimg = 0;
        int64_t mm = 0;
        while (e < nseg && h[e] * wd[e] == h[s] * wd[s]) { nimg += segs[e].n; mm += m[e]; ++e; }
        GCV_TRY(run("cnx.pool_ln", 2.0 * mm * C3, sizeof(T) * (double)mm * C3, [&] {
          if (one_fc)
            return launch_pool_ln<T>(Xc + moff[s] * C3, w.head_lnw, w.head_lnb, Pool, nimg, h[s] * wd[s], C3, 1e-6f, cur,
                                     segs[0].n, nseg, s);
          return launch_pool_ln<T>(Xc + moff[s] * C3, w.head_lnw, w.head_lnb, Pool + (int64_t)no * C3, nimg, h[s] * wd[s],
                                   C3, 1e-6f, cur);
        }));
      }
      if (!one_fc) {
        GemmArgs g{};
        g.A = Pool + (int64_t)no * C3; g.lda = C3; g.Wt = w.head_fc_w; g.C = segs[s].out; g.ldc = segs[s].out_ld;
        g.bias = w.head_fc_b; g.M = segs[s].n; g.N = 1000; g.K = C3; g.act = segs[s].act; g.splitk = 1;
        GCV_TRY(gemm("cnx.head_fc", g, A_PLAIN, EPI_BIAS_ACT));
        if (segs[s].pre) {
          g.C = segs[s].pre; g.act = ACT_NONE;
          GCV_TRY(gemm("explain.head_fc_pre", g, A_PLAIN, EPI_BIAS_ACT));
        }
      }
      no += segs[s].n;
    }
    if (tp) GCV_TRY(tap_bb(*tp, nseg, "pool", 3, 0, Pool, one_fc ? nseg : 0));
    if (one_fc) {
      GemmArgs g{};
      g.A = Pool; g.lda = C3; g.Wt = w.head_fc_w; g.C = segs[0].out; g.ldc = 1000;
      g.bias = w.head_fc_b; g.M = ntot; g.N = 1000; g.K = C3; g.act = segs[0].act; g.splitk = 1;
      GCV_TRY(gemm("cnx.head_fc", g, A_PLAIN, EPI_BIAS_ACT));
      if (segs[0].pre) {
        g.C = segs[0].pre; g.act = ACT_NONE;
        GCV_TRY(gemm("explain.head_fc_pre", g, A_PLAIN, EPI_BIAS_ACT));
      }
    }
    // explain: stage 3 has no LayerNorm-patchify epilogue, so its last block always leaves its output in X
    for (int s = 0; s < nseg; ++s)
      if (segs[s].s3) *segs[s].s3 = Xc + moff[s] * C3;
    if (!keep && !saving) arena.release(mk);
    return 0;
  }

  // keep_part (explain): receives the fc's split-K partials, which then stay allocated (the caller releases its own mark)
  int run_head(const HeadW<T>& hw, const T* feat, int B, int act, float* logits, const float** keep_part = nullptr) {
    // fc (2000 -> 500) eight ways split-K into fp32 partials; their sum, the bias, the activation and fc2 (500 -> 2) are one
    // small kernel (round 4: as one GEMM the layer was a chain of 32 K tiles on eight workgroups, 37 us at 128 rows)
    const int SK = 8, KPS = 256;
    const size_t mk = arena.mark();
    float* part = arena.get<float>((int64_t)SK * B * 500 + 8);
    GemmArgs g{};
    g.A = feat; g.lda = 2000; g.Wt = hw.fc_w; g.partial = part;
    g.M = B; g.N = 500; g.K = 2000; g.act = ACT_NONE; g.splitk = SK; g.k_per_split = KPS;
    GCV_TRY(gemm("head.fc", g, A_PLAIN, EPI_SPLITK));
    GCV_TRY(run("head.fc2", 2.0 * B * 2 * 500, 4.0 * (double)SK * B * 500, [&] {
      return launch_head_tail_splitk<T>(part, SK, hw.fc_b, act, hw.fc2_w, hw.fc2_b, logits, B, 500, cur);
    }));
    if (keep_part) *keep_part = part;
    else arena.release(mk);
    return 0;
  }

  // ------------------------------------------------------------ explain: Grad-CAM after the forward (cam.h)
  // part: the head's fc partials (8 ways, run_head); bbpre: (B, 2000) backbone logits before the activation; s3[p]: stage-3
  // tokens of pass p (hw[p] = side[p]^2 per image), their map at ex.cam + b * ex.cam_ld + off[p]
  int explain_tail(const CnxW<T>& bw, const HeadW<T>& hw, int act, int B, const float* part, const T* bbpre,
                   const float* logits, const T* const s3[2], const int hwp[2], const int side[2], const int off[2],
                   int up_pass, const Explain& ex, const Stage3In<T>* in3 = nullptr, const int* side2 = nullptr,
                   const char* net = nullptr) {
    const int C3 = cnx_arch(arch).dims[3];
    float* dfeat = arena.get<float>((int64_t)B * 2000);
    float* dpool = arena.get<float>((int64_t)B * 2 * C3);
    if (!arena.dry && arena.overflow) { set_error("workspace arena too small"); return -6; }
    HeadBwdArgs ha{part, 8, hw.fc_b, hw.fc2_w, logits, ex.target, hw.fc_w, bbpre, dfeat, B, act};
    GCV_TRY(run("explain.head_bwd", 2.0 * B * 500 * 2000, sizeof(T) * (500.0 * 2000 + 2.0 * B * 2000) + 4.0 * B * (8 * 500 + 2000),
                [&] { return launch_head_bwd<T>(ha, cur); }));
    GCV_TRY(run("explain.bb_fc_bwd", 2.0 * 2 * B * 1000 * C3, sizeof(T) * 1000.0 * C3 + 4.0 * B * (2000 + 2 * C3),
                [&] { return launch_bb_bwd<T>(dfeat, bw.head_fc_w, dpool, 2 * B, C3, cur); }));
    if (ex.layer == 2) return explain_tail_s2(bw, B, dpool, s3, side, side2, up_pass, ex, in3, net);
    CamArgs ca{};
    for (int q = 0; q < 2; ++q) { ca.A[q] = s3[q]; ca.hw[q] = hwp[q]; ca.side[q] = side[q]; ca.cam_off[q] = off[q]; }
    ca.npass = 2; ca.cam_ld = ex.cam_ld; ca.up_pass = up_pass; ca.lnw = bw.head_lnw; ca.dpool = dpool;
    ca.cam = ex.cam; ca.cam224 = ex.cam224; ca.eps = 1e-6f; ca.B = B;
    GCV_TRY(run("explain.cam", 4.0 * B * (hwp[0] + hwp[1]) * C3, sizeof(T) * (double)B * (hwp[0] + hwp[1]) * C3 +
                (ex.cam224 ? 4.0 * B * 224 * 224 : 0.0), [&] { return launch_cam<T>(ca, C3, cur); }));
    return 0;
  }

  // Grad-CAM at the output of stage 2 (cam_bwd.h): dpool (B, 2, C3) -> backward through pool + LayerNorm, stage 3's blocks
  // and the down-sampling -> d A2 -> alpha, maps.  side3[p] / side2[p]: stage-3 / stage-2 map side of pass p; in3[p]: what
  // the pass kept.  Gradient rows: pass 0's tokens, then pass 1's.  Maps of (b, p) at ex.cam + b * ex.cam_ld + (p ? side2[0]^2 : 0).
  int explain_tail_s2(const CnxW<T>& bw, int B, const float* dpool, const T* const s3[2], const int side3[2],
                      const int side2[2], int up_pass, const Explain& ex, const Stage3In<T>* in3, const char* net) {
    const CnxArch& A = cnx_arch(arch);
    const int C3 = A.dims[3], C2 = A.dims[2], nb = A.depths[3];
    GCV_REQUIRE(in3 && side2 && net && nb == 3, "stage-3 inputs were not kept");
    int hw3[2], tok0[2];
    int64_t M = 0, M2 = 0, tok2[2];
    for (int p = 0; p < 2; ++p) {
      GCV_REQUIRE(side2[p] / 2 == side3[p], "stage-2 / stage-3 map sides");
      hw3[p] = side3[p] * side3[p];
      tok0[p] = (int)M; tok2[p] = M2;
      M += (int64_t)B * hw3[p];
      M2 += (int64_t)B * side2[p] * side2[p];
    }
    GCV_REQUIRE(M * 4 * C3 < (int64_t)1 << 31, "token count too large for 32-bit GEMM indexing");
    float* G = arena.get<float>(M * C3);             // d logit / d (block output), then d (block input), in place
    T* Gt = arena.get<T>(M * C3);                    // its row-scaled copy in T: the GEMM operand
    float* invA = arena.get<float>(M + 8);
    float* invB = arena.get<float>(M + 8);
    float* Dh = arena.get<float>(M * 4 * C3);        // dz . W2 (M, 4 C3); later dx0 . W_down (M, 4 C2)
    T* Pre = arena.get<T>(M * 4 * C3);               // hidden pre-activation, then dh * GELU' in place
    T* Yb = arena.get<T>(M * C3);                    // the block's LayerNorm output, recomputed
    float* Dl = arena.get<float>(M * C3);            // dpre . W1
    float* Dw = arena.get<float>(M * C3);            // d (raw depthwise output)
    float* dA2 = arena.get<float>(M2 * C2);
    float* alpha = arena.get<float>((int64_t)2 * B * C2);
    if (!arena.dry && arena.overflow) { set_error("workspace arena too small"); return -6; }

    PoolLnBwdArgs pa{};
    for (int p = 0; p < 2; ++p) { pa.A[p] = s3[p]; pa.hw[p] = hw3[p]; pa.tok0[p] = tok0[p]; }
    pa.npass = 2; pa.B = B; pa.lnw = bw.head_lnw; pa.dpool = dpool; pa.dA = G; pa.eps = 1e-6f;
    GCV_TRY(run("explain2.pool_ln_bwd", 4.0 * M * C3, (sizeof(T) + 4.0) * (double)M * C3,
                [&] { return launch_pool_ln_bwd<T>(pa, C3, cur); }));
    auto dgemm = [&](const char* tag, const T* a, const T* wt, float* out, int N, int K) {
      GemmArgs g{};
      g.A = a; g.lda = K; g.Wt = wt; g.partial = out; g.M = (int)M; g.N = N; g.K = K; g.act = ACT_NONE;
      g.splitk = 1; g.k_per_split = K;
      return gemm(tag, g, A_PLAIN, EPI_SPLITK);
    };
    int bi = A.nblocks() - nb;
    for (int j = nb - 1; j >= 0; --j) {
      const CnxBlockW<T>& k = bw.blk[bi + j];
      GCV_TRY(run("explain2.scale_rows", 2.0 * M * C3, (sizeof(T) + 4.0) * (double)M * C3,
                  [&] { return launch_scale_rows<T>(G, k.mlp.gamma, Gt, invA, (int)M, C3, cur); }));
      GCV_TRY(dgemm("explain2.dz_w2", Gt, bw.bwd_w2t[j], Dh, 4 * C3, C3));
      // the forward keeps neither the LayerNorm output nor the hidden pre-activation: the forward's own kernels again,
      // in the forward's launch shape (both passes in one launch where their tokens are neighbours of one geometry)
      const bool one = side3[0] == side3[1] && in3[1].x[j] == in3[0].x[j] + (int64_t)B * hw3[0] * C3;
      for (int p = 0; p < (one ? 1 : 2); ++p) {
        const int nimg = one ? 2 * B : B;
        GCV_TRY(run("explain2.dwconv7_ln", 2.0 * 49 * nimg * hw3[p] * C3, 2.0 * sizeof(T) * (double)nimg * hw3[p] * C3, [&] {
          return launch_dwconv7_ln<T>(in3[p].x[j], k.dw_w, k.dw_b, k.ln_w, k.ln_b, Yb + (int64_t)tok0[p] * C3, nimg, side3[p],
                                      side3[p], C3, 1e-6f, cur);
        }));
      }
      {
        GemmArgs g{};
        g.A = Yb; g.lda = C3; g.Wt = k.mlp.w1; g.C = Pre; g.ldc = 4 * C3; g.bias = k.mlp.b1;
        g.M = (int)M; g.N = 4 * C3; g.K = C3; g.act = ACT_NONE; g.splitk = 1;
        GCV_TRY(gemm("explain2.pw1_pre", g, A_PLAIN, EPI_BIAS_ACT));
      }
      GCV_TRY(run("explain2.gelu_bwd", 12.0 * M * 4 * C3, (2.0 * sizeof(T) + 4.0) * (double)M * 4 * C3,
                  [&] { return launch_gelu_bwd<T>(Dh, invA, Pre, invB, (int)M, 4 * C3, cur); }));
      GCV_TRY(dgemm("explain2.dpre_w1", Pre, bw.bwd_w1t[j], Dl, C3, 4 * C3));
      for (int p = 0; p < 2; ++p) {
        DwLnBwdArgs da{in3[p].x[j], k.dw_w, k.dw_b, k.ln_w, Dl + (int64_t)tok0[p] * C3, invB + tok0[p],
                       Dw + (int64_t)tok0[p] * C3, B, side3[p], 1e-6f};
        GCV_TRY(run("explain2.dw_ln_bwd", 2.0 * 49 * B * hw3[p] * C3, (sizeof(T) + 8.0) * (double)B * hw3[p] * C3,
                    [&] { return launch_dw_ln_bwd<T>(da, C3, cur); }));
        GCV_TRY(run("explain2.dw_dgrad_res", 2.0 * 49 * B * hw3[p] * C3, 12.0 * (double)B * hw3[p] * C3, [&] {
          return launch_dw_dgrad_res(Dw + (int64_t)tok0[p] * C3, k.dw_w, G + (int64_t)tok0[p] * C3, B, side3[p], C3, cur);
        }));
      }
    }
    GCV_TRY(run("explain2.scale_rows", 2.0 * M * C3, (sizeof(T) + 4.0) * (double)M * C3,
                [&] { return launch_scale_rows<T>(G, nullptr, Gt, invA, (int)M, C3, cur); }));
    GCV_TRY(dgemm("explain2.dx_wdown", Gt, bw.bwd_downt, Dh, 4 * C2, C3));
    Cam2Args ca{};
    for (int p = 0; p < 2; ++p) {
      DownLnBwdArgs da{in3[p].s2, bw.down[2].ln_w, Dh + (int64_t)tok0[p] * 4 * C2, invA + tok0[p], dA2 + tok2[p] * C2, B,
                       side2[p], 1e-6f};
      GCV_TRY(run("explain2.down_ln_bwd", 10.0 * B * side2[p] * side2[p] * C2, (sizeof(T) + 8.0) * (double)B * side2[p] * side2[p] * C2,
                  [&] { return launch_down_ln_bwd<T>(da, C2, cur); }));
      ca.A[p] = in3[p].s2; ca.dA2[p] = dA2 + tok2[p] * C2; ca.side[p] = side2[p];
      ca.cam_off[p] = p ? side2[0] * side2[0] : 0;
    }
    ca.npass = 2; ca.cam_ld = ex.cam_ld; ca.up_pass = up_pass; ca.B = B; ca.cam = ex.cam; ca.cam224 = ex.cam224; ca.alpha = alpha;
    GCV_TRY(run("explain2.cam", 4.0 * M2 * C2, (sizeof(T) + 4.0) * (double)M2 * C2 + (ex.cam224 ? 4.0 * B * 224 * 224 : 0.0),
                [&] { return launch_cam2<T>(ca, C2, cur); }));
    if (!taps.empty()) GCV_TRY(tap_net((std::string(net) + ".explain.alpha2").c_str(), alpha, (size_t)2 * B * C2 * sizeof(float)));
    return 0;
  }

  int check_batch(int B) {
    GCV_REQUIRE(B >= 1, "batch must be >= 1");
    GCV_REQUIRE(B <= max_batch, "batch exceeds the max_batch this handle was created with");
    return 0;
  }

  // ------------------------------------------------------------ ED (model/genconvit_ed.py:77-88)
  int ed_forward(const void* xv, int B, float* logits, hipStream_t s) override { return ed_run(xv, B, logits, s, nullptr); }
  int ed_explain(const void* xv, int B, float* logits, const Explain& ex, hipStream_t s) override {
    return ed_run(xv, B, logits, s, &ex);
  }
  // ex: explain request (null: the plain forward, whose launches it leaves untouched)
  int ed_run(const void* xv, int B, float* logits, hipStream_t s, const Explain* ex) {
    if (!arena.dry) {
      GCV_REQUIRE(has_ed, "ED weights not loaded (gcv_load_ed)");
      GCV_TRY(check_batch(B));
      GCV_REQUIRE(xv && logits, "null input/output");
      GCV_REQUIRE(!ex || ex->cam, "null map output");
    }
    GCV_REQUIRE(!ex || ex->layer == 2 || ex->layer == 3, "explain layer must be 2 or 3");
    cur = s;
    const T* x = (const T*)xv;
    if (!taps.empty()) tap_reset("ed");
    const ArenaScope scope(arena);
    T* e1 = arena.get<T>((int64_t)B * 112 * 112 * 16);
    T* e2 = arena.get<T>((int64_t)B * 56 * 56 * 32);
    T* e3 = arena.get<T>((int64_t)B * 28 * 28 * 64);
    T* e4 = arena.get<T>((int64_t)B * 14 * 14 * 128);
    T* e5 = arena.get<T>((int64_t)B * 7 * 7 * 256);
    T* d1 = arena.get<T>((int64_t)B * 14 * 14 * 128);
    T* d2 = arena.get<T>((int64_t)B * 28 * 28 * 64);
    T* d3 = arena.get<T>((int64_t)B * 56 * 56 * 32);
    T* d4 = arena.get<T>((int64_t)B * 112 * 112 * 16);
    T* rec = arena.get<T>((int64_t)B * 224 * 224 * 3);
    T* feat = arena.get<T>((int64_t)B * 2000);
    T* bbpre = ex ? arena.get<T>((int64_t)B * 2000) : nullptr;
    if (!arena.dry && arena.overflow) { set_error("workspace arena too small"); return -6; }

    GCV_TRY(run("ed.enc1_conv3_relu_pool", 2.0 * B * 224 * 224 * 16 * 27,
                sizeof(T) * (double)B * (3 * 224 * 224 + 16 * 112 * 112), [&] {
      return launch_conv3_first<T>(x, 3 * 224 * 224, 224 * 224, 224, 1, ed.enc1_w, ed.enc1_b, e1, B, 224, 224, true,
                                   ACT_RELU, cur);
    }));
    {
      const T* in[4] = {e1, e2, e3, e4};
      T* out[4] = {e2, e3, e4, e5};
      const int Hs[4] = {112, 56, 28, 14};
      const int cl[4] = {4, 5, 6, 7};
      for (int l = 0; l < 4; ++l) {
        GemmArgs g{};
        g.A = in[l]; g.Wt = ed.enc_w[l]; g.C = out[l]; g.bias = ed.enc_b[l];
        g.M = B * Hs[l] * Hs[l]; g.N = 2 << cl[l]; g.K = 9 << cl[l]; g.ldc = g.N; g.act = ACT_RELU; g.splitk = 1;
        g.H = Hs[l]; g.W = Hs[l]; g.cin_log2 = cl[l];
        GCV_TRY(gemm("ed.enc_conv3_relu_pool", g, A_IM2COL3_POOL, EPI_POOL4));
      }
    }
    {
      const T* in[4] = {e5, d1, d2, d3};
      T* out[4] = {d1, d2, d3, d4};
      const int Hs[4] = {7, 14, 28, 56};
      const int col[4] = {7, 6, 5, 4};   // log2(Cout)
      for (int l = 0; l < 4; ++l) {
        GemmArgs g{};
        g.A = in[l]; g.lda = 2 << col[l]; g.Wt = ed.dec_w[l]; g.C = out[l]; g.bias = ed.dec_b[l];
        g.M = B * Hs[l] * Hs[l]; g.N = 4 << col[l]; g.K = 2 << col[l]; g.act = ACT_RELU; g.splitk = 1;
        g.H = Hs[l]; g.W = Hs[l]; g.cout_log2 = col[l];
        GCV_TRY(gemm("ed.dec_convT_relu", g, A_PLAIN, EPI_CONVT));
      }
    }
    GCV_TRY(run("ed.dec5_convT_relu", 2.0 * B * 112 * 112 * 16 * 12,
                sizeof(T) * (double)B * (16 * 112 * 112 + 3 * 224 * 224),
                [&] { return launch_convt2_small<T>(d4, ed.dec5_w, ed.dec5_b, rec, B, 112, 112, ACT_RELU, cur); }));
    // both backbone passes share weights and shape -> one 2B-image token stream (running backbone(orig) on a side stream
    // under the encoder / decoder chain instead, as the VAE does, measured 8.69 vs 8.25 ms per step: the merged launches
    // are worth more than the overlap).  cat order (genconvit_ed.py:85): [backbone(recon), backbone(orig)], GELU (:75)
    Seg<T> segs[2];
    segs[0] = Seg<T>{rec, (int64_t)224 * 224 * 3, 1, 224 * 3, 3, B, 224, 224, feat, 2000, ACT_GELU};
    segs[1] = Seg<T>{x, (int64_t)3 * 224 * 224, 224 * 224, 224, 1, B, 224, 224, feat + 1000, 2000, ACT_GELU};
    const T* s3[2] = {nullptr, nullptr};
    Stage3In<T> in3[2];
    const float* head_part = nullptr;
    if (ex)
      for (int q = 0; q < 2; ++q) {
        segs[q].pre = bbpre + 1000 * q; segs[q].s3 = &s3[q];
        if (ex->layer == 2) segs[q].in3 = &in3[q];
      }
    const TapPass tp{"ed", 2, 0, {B, B}, {224, 224}, {224, 224}};
    GCV_TRY(run_convnext(bb_ed, segs, 2, false, taps.empty() ? nullptr : &tp));
    GCV_TRY(run_head(ed.head, feat, B, ACT_GELU, logits, ex ? &head_part : nullptr));
    if (ex) {
      // maps [b][pass][7][7], passes in cat order (reconstruction, original); the original frame's map is upsampled
      // (at stage 2: [b][pass][14][14])
      const int hwp[2] = {49, 49}, side[2] = {7, 7}, off[2] = {0, 49}, side2[2] = {14, 14};
      GCV_TRY(explain_tail(bb_ed, ed.head, ACT_GELU, B, head_part, bbpre, logits, s3, hwp, side, off, 1, *ex, in3, side2, "ed"));
    }
    if (!taps.empty()) {
      const T* et[5] = {e1, e2, e3, e4, e5};
      const int64_t ee[5] = {112 * 112 * 16, 56 * 56 * 32, 28 * 28 * 64, 14 * 14 * 128, 7 * 7 * 256};
      const T* dt[4] = {d1, d2, d3, d4};
      const int64_t de[4] = {14 * 14 * 128, 28 * 28 * 64, 56 * 56 * 32, 112 * 112 * 16};
      for (int l = 0; l < 5; ++l) GCV_TRY(tap_net(("ed.e" + std::to_string(l + 1)).c_str(), et[l], B * ee[l] * sizeof(T)));
      for (int l = 0; l < 4; ++l) GCV_TRY(tap_net(("ed.d" + std::to_string(l + 1)).c_str(), dt[l], B * de[l] * sizeof(T)));
      GCV_TRY(tap_net("ed.rec", rec, (size_t)B * 224 * 224 * 3 * sizeof(T)));
      GCV_TRY(tap_net("ed.feat", feat, (size_t)B * 2000 * sizeof(T)));
    }
    return 0;
  }

  // ------------------------------------------------------------ VAE (model/genconvit_vae.py:107-116)
  int vae_forward(const void* xv, const float* eps, int B, float* logits, void* recon224, float* mse, float* kl,
                  hipStream_t s) override {
    return vae_run(xv, eps, B, logits, recon224, mse, kl, s, nullptr);
  }
  int vae_explain(const void* xv, const float* eps, int B, float* logits, const Explain& ex, hipStream_t s) override {
    return vae_run(xv, eps, B, logits, nullptr, nullptr, nullptr, s, &ex);
  }
  int vae_run(const void* xv, const float* eps, int B, float* logits, void* recon224, float* mse, float* kl,
              hipStream_t s, const Explain* ex) {
    if (!arena.dry) {
      GCV_REQUIRE(has_vae, "VAE weights not loaded (gcv_load_vae)");
      GCV_TRY(check_batch(B));
      GCV_REQUIRE(xv && eps && logits, "null input/eps/output");
      GCV_REQUIRE(!kl || vae.var_w, "KL requested but encoder.var weights were not loaded");
      GCV_REQUIRE(!ex || ex->cam, "null map output");
    }
    GCV_REQUIRE(!ex || ex->layer == 2 || ex->layer == 3, "explain layer must be 2 or 3");
    cur = s;
    const T* x = (const T*)xv;
    if (!taps.empty()) tap_reset("vae");
    // split-K plan of the 25088-deep mu / var GEMMs (392 K tiles of 64 = 8 * 49): 8 ways at 128-row tiles (98 x 8 = 784
    // workgroups), 7 ways for batches of 64 frames and fewer, whose 32- / 64-row tiles leave room for every one of the 686
    // workgroups at once (vae B = 32 bf16, same box: 0.143 -> 0.118 ms; at B = 128 seven ways measure 0.193 against 0.175)
    const int SPLITK = B <= 64 ? 7 : 8, KPS = 25088 / SPLITK;
    const ArenaScope scope(arena);
    T* v1 = arena.get<T>((int64_t)B * 112 * 112 * 16);
    T* v2 = arena.get<T>((int64_t)B * 56 * 56 * 32);
    T* v3 = arena.get<T>((int64_t)B * 28 * 28 * 64);
    T* v4 = arena.get<T>((int64_t)B * 14 * 14 * 128);
    float* part = arena.get<float>((int64_t)8 * B * 12544);
    float* mu = arena.get<float>((int64_t)B * 12544);
    float* rowsum = arena.get<float>(B + 8);
    T* z = arena.get<T>((int64_t)B * 12544);
    T* d1 = arena.get<T>((int64_t)B * 14 * 14 * 64);
    T* d2 = arena.get<T>((int64_t)B * 28 * 28 * 32);
    T* d3 = arena.get<T>((int64_t)B * 56 * 56 * 16);
    T* xhat = arena.get<T>((int64_t)B * 112 * 112 * 3);
    T* feat = arena.get<T>((int64_t)B * 2000);
    float* msepart = arena.get<float>((int64_t)B * 196);
    T* bbpre = ex ? arena.get<T>((int64_t)B * 2000) : nullptr;
    if (!arena.dry && arena.overflow) { set_error("workspace arena too small"); return -6; }

    // cat order (genconvit_vae.py:113): [backbone(x @224), backbone(x_hat @112)], activation ReLU (:104)
    Seg<T> segs[2];
    segs[0] = Seg<T>{x, (int64_t)3 * 224 * 224, 224 * 224, 224, 1, B, 224, 224, feat, 2000, ACT_RELU};
    segs[1] = Seg<T>{xhat, (int64_t)112 * 112 * 3, 1, 112 * 3, 3, B, 112, 112, feat + 1000, 2000, ACT_RELU};
    const T* s3[2] = {nullptr, nullptr};
    Stage3In<T> in3[2];
    const float* head_part = nullptr;
    if (ex)
      for (int q = 0; q < 2; ++q) {
        segs[q].pre = bbpre + 1000 * q; segs[q].s3 = &s3[q];
        if (ex->layer == 2) segs[q].in3 = &in3[q];
      }
    const bool split = (vae_split_env >= 0 ? vae_split_env != 0 : !in_ensemble) && !prof.enabled;   // (profiled steps stay on one stream: serial per-kernel times)
    const TapPass tp0{"vae", 2, 0, {B, B}, {224, 112}, {224, 112}}, tp1{"vae", 2, 1, {B, B}, {224, 112}, {224, 112}};
    const bool tapping = !taps.empty();
    Join join;
    if (split) GCV_TRY(side_pass(bb_vae, &segs[0], s, join, tapping ? &tp0 : nullptr));

    GCV_TRY(run("vae.enc1_conv3s2_bn_leaky", 2.0 * B * 112 * 112 * 16 * 27,
                sizeof(T) * (double)B * (3 * 224 * 224 + 16 * 112 * 112), [&] {
      return launch_conv3_first<T>(x, 3 * 224 * 224, 224 * 224, 224, 1, vae.enc1_w, vae.enc1_b, v1, B, 224, 224,
                                   false, ACT_LEAKY, cur);
    }));
    {
      const T* in[3] = {v1, v2, v3};
      T* out[3] = {v2, v3, v4};
      const int Hs[3] = {112, 56, 28};
      const int cl[3] = {4, 5, 6};
      for (int l = 0; l < 3; ++l) {
        GemmArgs g{};
        g.A = in[l]; g.Wt = vae.enc_w[l]; g.C = out[l]; g.bias = vae.enc_b[l];
        g.M = B * (Hs[l] / 2) * (Hs[l] / 2); g.N = 2 << cl[l]; g.K = 9 << cl[l]; g.ldc = g.N; g.act = ACT_LEAKY;
        g.splitk = 1; g.H = Hs[l]; g.W = Hs[l]; g.cin_log2 = cl[l];
        GCV_TRY(gemm("vae.enc_conv3s2_bn_leaky", g, A_IM2COL3_S2, EPI_BIAS_ACT));
      }
    }
    {
      GemmArgs g{};
      g.A = v4; g.lda = 25088; g.Wt = vae.mu_w; g.partial = part; g.M = B; g.N = 12544; g.K = 25088;
      g.splitk = SPLITK; g.k_per_split = KPS; g.act = ACT_NONE;
      GCV_TRY(gemm("vae.mu_gemm_splitk", g, A_PLAIN, EPI_SPLITK));
      GCV_TRY(run("vae.reparam", 4.0 * B * 12544, 4.0 * (SPLITK + 2) * (double)B * 12544, [&] {
        return launch_reparam<T>(part, SPLITK, vae.mu_b, eps, mu, z, B, 12544, cur);
      }));
      if (kl) {
        g.Wt = vae.var_w;
        GCV_TRY(gemm("vae.var_gemm_splitk", g, A_PLAIN, EPI_SPLITK));
        GCV_TRY(run("vae.kl", 6.0 * B * 12544, 4.0 * (SPLITK + 1) * (double)B * 12544,
                    [&] { return launch_kl(part, SPLITK, vae.var_b, mu, rowsum, kl, B, 12544, cur); }));
      }
    }
    {
      const T* in[3] = {z, d1, d2};
      T* out[3] = {d1, d2, d3};
      const int Hs[3] = {7, 14, 28};
      const int cin[3] = {256, 64, 32};
      const int col[3] = {6, 5, 4};
      for (int l = 0; l < 3; ++l) {
        GemmArgs g{};
        g.A = in[l]; g.lda = cin[l]; g.Wt = vae.dec_w[l]; g.C = out[l]; g.bias = vae.dec_b[l];
        g.M = B * Hs[l] * Hs[l]; g.N = 4 << col[l]; g.K = cin[l]; g.act = ACT_LEAKY; g.splitk = 1;
        g.H = Hs[l]; g.W = Hs[l]; g.cout_log2 = col[l];
        GCV_TRY(gemm("vae.dec_convT_leaky", g, A_PLAIN, EPI_CONVT));
      }
    }
    GCV_TRY(run("vae.dec4_convT_leaky", 2.0 * B * 56 * 56 * 16 * 12,
                sizeof(T) * (double)B * (16 * 56 * 56 + 3 * 112 * 112),
                [&] { return launch_convt2_small<T>(d3, vae.dec4_w, vae.dec4_b, xhat, B, 56, 56, ACT_LEAKY, cur); }));
    if (after_chain && !arena.dry) GCV_TRY(after_chain());
    if (split) { GCV_TRY(run_convnext(bb_vae, &segs[1], 1, true, tapping ? &tp1 : nullptr)); }
    else { GCV_TRY(run_convnext(bb_vae, segs, 2, false, tapping ? &tp0 : nullptr)); }
    join.now();
    if (tapping) {
      const T* vt[4] = {v1, v2, v3, v4};
      const int64_t ve[4] = {112 * 112 * 16, 56 * 56 * 32, 28 * 28 * 64, 14 * 14 * 128};
      const T* dt[3] = {d1, d2, d3};
      const int64_t de[3] = {14 * 14 * 64, 28 * 28 * 32, 56 * 56 * 16};
      for (int l = 0; l < 4; ++l) GCV_TRY(tap_net(("vae.v" + std::to_string(l + 1)).c_str(), vt[l], B * ve[l] * sizeof(T)));
      GCV_TRY(tap_net("vae.mu", mu, (size_t)B * 12544 * sizeof(float)));
      GCV_TRY(tap_net("vae.z", z, (size_t)B * 12544 * sizeof(T)));
      for (int l = 0; l < 3; ++l) GCV_TRY(tap_net(("vae.d" + std::to_string(l + 1)).c_str(), dt[l], B * de[l] * sizeof(T)));
      GCV_TRY(tap_net("vae.xhat", xhat, (size_t)B * 112 * 112 * 3 * sizeof(T)));
      GCV_TRY(tap_net("vae.feat", feat, (size_t)B * 2000 * sizeof(T)));
    }
    GCV_TRY(run_head(vae.head, feat, B, ACT_RELU, logits, ex ? &head_part : nullptr));
    if (ex) {
      // maps [b][7 x 7 of the original frame, 3 x 3 of x_hat at 112]; the original frame's map is upsampled
      // (at stage 2: [b][14 x 14, 7 x 7])
      const int hwp[2] = {49, 9}, side[2] = {7, 3}, off[2] = {0, 49}, side2[2] = {14, 7};
      GCV_TRY(explain_tail(bb_vae, vae.head, ACT_RELU, B, head_part, bbpre, logits, s3, hwp, side, off, 0, *ex, in3, side2, "vae"));
    }
    if (recon224 || mse) {
      GCV_TRY(run("vae.resize_mse", 30.0 * B * 224 * 224, sizeof(T) * (double)B * (3 * 112 * 112 + 6 * 224 * 224), [&] {
        return launch_resize_mse<T>(xhat, x, (T*)recon224, msepart, mse, B, cur);
      }));
    }
    return 0;
  }

  // standalone backbone pass (unit parity / A5): x NCHW (B,3,res,res) -> (B,1000) in T
  int convnext_forward(int which, const void* xv, int B, int res, void* logits1000, hipStream_t s) override {
    GCV_REQUIRE(which == 0 ? has_ed : has_vae, "backbone weights not loaded");
    GCV_TRY(check_batch(B));
    GCV_REQUIRE(cnx_res_ok(arch, res), cnx_res_rule(arch));
    cur = s;
    const ArenaScope scope(arena);
    Seg<T> seg{(const T*)xv, (int64_t)3 * res * res, (int64_t)res * res, res, 1, B, res, res, (T*)logits1000, 1000, ACT_NONE};
    return run_convnext(which == 0 ? bb_ed : bb_vae, &seg, 1);
  }

  int swin_forward(const void* xv, int B, void* logits1000, hipStream_t s) override {
    if (!arena.dry) {
      GCV_REQUIRE(has_swin, "Swin weights not loaded (gcv_load_swin)");
      GCV_TRY(check_batch(B));
    }
    cur = s;
    if (!arena.dry) GCV_REQUIRE(xv && logits1000, "null input/output");
    const ArenaScope scope(arena);
    return run_swin<T>(*this, swin, (const T*)xv, B, (T*)logits1000);
  }

  int init() override {
    GCV_CHECK_HIP(hipSetDevice(device));
    arena.dry = true;
    arena.off = arena.peak = 0;
    // the explain variants keep the head's inputs alive on top of the forward's buffers: the arena holds them too
    // (at either layer: stage 2's keeps stage 3's inputs and the backward's gradient buffers as well)
    int rc = 0;
    for (int layer = 3; layer >= 2 && !rc; --layer) {
      Explain ex;
      ex.layer = layer;
      rc = ed_run(nullptr, max_batch, nullptr, nullptr, &ex);
      if (!rc) rc = vae_run(nullptr, nullptr, max_batch, nullptr, nullptr, nullptr, nullptr, nullptr, &ex);
      in_ensemble = true;                  // both VAE schedules (see vae_split_env): the arena holds the larger footprint
      if (!rc) rc = vae_run(nullptr, nullptr, max_batch, nullptr, nullptr, nullptr, nullptr, nullptr, &ex);
      in_ensemble = false;
    }
    if (!rc) rc = swin_forward(nullptr, max_batch, nullptr, nullptr);
    arena.dry = false;
    if (rc) return rc;
    arena.cap = arena.peak + 4096;
    arena.off = 0;
    GCV_CHECK_HIP(hipMalloc((void**)&arena.base, arena.cap));
    return 0;
  }
};

}  // namespace gcv
