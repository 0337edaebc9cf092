"""ctypes binding of ``libgenconvit_hip.so`` (C ABI: include/genconvit_hip.h).

The north-star asks for cffi; cffi is not installed in this image, ctypes (stdlib) binds the same
C ABI.  There is NO CPU fallback: if the library is missing, or there is no gfx950 device, the
calls raise.

The library is linked without a hard dependency on a particular HIP runtime (``-no-hip-rt``):
PyTorch-ROCm wheels bundle their own ``libamdhip64.so`` and a second runtime instance in the same
process would not understand torch's streams.  So the runtime already used by the process is made
globally visible first (torch's bundled copy when torch is importable, /opt/rocm's otherwise).
"""
from __future__ import annotations

import ctypes
import ctypes.util
import json
import os
import threading

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("GCV_LIB_PATH") or os.path.join(_HERE, "lib", "libgenconvit_hip.so")   # override: diagnostic builds

GCV_F32, GCV_BF16, GCV_F16 = 0, 1, 2
ACT_NONE, ACT_RELU, ACT_GELU, ACT_LEAKY = 0, 1, 2, 3
A_PLAIN, A_IM2COL3_POOL, A_IM2COL3_S2 = 0, 1, 2
EPI_BIAS_ACT, EPI_RESID, EPI_POOL4, EPI_CONVT, EPI_SPLITK = 0, 1, 2, 3, 4

c_void_p, c_int, c_int64, c_float, c_char_p, c_size_t = (ctypes.c_void_p, ctypes.c_int, ctypes.c_int64,
                                                         ctypes.c_float, ctypes.c_char_p, ctypes.c_size_t)


class TensorDesc(ctypes.Structure):
    _fields_ = [("name", c_char_p), ("data", c_void_p), ("numel", c_int64), ("on_device", c_int)]


class GemmArgs(ctypes.Structure):
    _fields_ = [("A", c_void_p), ("Wt", c_void_p), ("C", c_void_p), ("bias", c_void_p), ("gamma", c_void_p),
                ("resid", c_void_p), ("partial", c_void_p)] + \
               [(n, c_int) for n in ("M", "N", "K", "lda", "ldc", "act", "splitk", "k_per_split", "H", "W",
                                     "cin_log2", "cout_log2")]


# every symbol include/genconvit_hip.h declares: name -> (restype, argtypes)
SIGNATURES = {
    "gcv_last_error": (c_char_p, []),
    "gcv_create": (c_int, [ctypes.POINTER(c_void_p), c_int, c_int, c_int]),
    "gcv_create_arch": (c_int, [ctypes.POINTER(c_void_p), c_int, c_int, c_int, c_int]),
    "gcv_handle_arch": (c_int, [c_void_p]),
    "gcv_destroy": (None, [c_void_p]),
    "gcv_workspace_bytes": (c_size_t, [c_void_p]),
    "gcv_load_ed": (c_int, [c_void_p, ctypes.POINTER(TensorDesc), c_int]),
    "gcv_load_vae": (c_int, [c_void_p, ctypes.POINTER(TensorDesc), c_int]),
    "gcv_load_swin": (c_int, [c_void_p, ctypes.POINTER(TensorDesc), c_int, c_char_p]),
    "gcv_ed_forward": (c_int, [c_void_p, c_void_p, c_int, c_void_p, c_void_p]),
    "gcv_vae_forward": (c_int, [c_void_p, c_void_p, c_void_p, c_int, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p]),
    "gcv_genconvit_forward": (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_int, c_void_p, c_void_p]),
    "gcv_ed_explain": (c_int, [c_void_p, c_void_p, c_int, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p]),
    "gcv_vae_explain": (c_int, [c_void_p, c_void_p, c_void_p, c_int, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p]),
    "gcv_genconvit_explain": (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_int, c_void_p, c_void_p, c_void_p,
                                      c_void_p, c_void_p]),
    "gcv_ed_explain_at": (c_int, [c_void_p, c_void_p, c_int, c_void_p, c_int, c_void_p, c_void_p, c_void_p, c_void_p]),
    "gcv_vae_explain_at": (c_int, [c_void_p, c_void_p, c_void_p, c_int, c_void_p, c_int, c_void_p, c_void_p, c_void_p,
                                   c_void_p]),
    "gcv_genconvit_explain_at": (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_int, c_void_p, c_int, c_void_p, c_void_p,
                                         c_void_p, c_void_p]),
    "gcv_comm_available": (c_int, []),
    "gcv_comm_count": (c_int, [c_void_p]),
    "gcv_comm_unique_id": (c_int, [c_void_p]),
    "gcv_comm_create": (c_int, [ctypes.POINTER(c_void_p), c_int, c_int, c_void_p, c_int]),
    "gcv_comm_destroy": (None, [c_void_p]),
    "gcv_allgather_logits": (c_int, [c_void_p, c_void_p, c_int, c_void_p, c_void_p]),
    "gcv_convnext_forward": (c_int, [c_void_p, c_int, c_void_p, c_int, c_int, c_void_p, c_void_p]),
    "gcv_swin_forward": (c_int, [c_void_p, c_void_p, c_int, c_void_p, c_void_p]),
    "gcv_vote": (c_int, [c_void_p, c_int, c_void_p, c_void_p]),
    "gcv_preprocess": (c_int, [c_int, c_void_p, c_void_p, c_int, c_int, c_int, c_void_p]),
    "gcv_face_crop_resize": (c_int, [c_void_p, c_int, c_int, c_int, c_void_p, c_int, c_void_p, c_int, c_void_p]),
    "gcv_face_crop_preprocess": (c_int, [c_int, c_void_p, c_int, c_int, c_int, c_void_p, c_int, c_void_p, c_int, c_void_p]),
    "gcv_cam_overlay": (c_int, [c_void_p, c_int, c_int, c_int, c_void_p, c_int, c_void_p, c_int, c_int, c_void_p, c_float,
                                c_int, c_void_p, c_void_p]),
    "gcv_scan_annotate": (c_int, [c_void_p, c_int, c_int, c_int, c_void_p, c_void_p, c_int, c_void_p, c_int, c_int, c_int,
                                  c_void_p, c_void_p]),
    "gcv_yuv420_to_rgb": (c_int, [c_void_p, c_int, c_int, c_int, c_int, c_int, c_int, c_void_p, c_void_p]),
    "gcv_rgb_to_yuv420": (c_int, [c_void_p, c_int, c_int, c_int, c_int, c_int, c_int, c_void_p, c_void_p]),
    "gcv_track_match": (c_int, [c_void_p, c_int, c_int, c_int, c_void_p, c_int, c_int, c_int, c_void_p, c_void_p]),
    "gcv_track_chain": (c_int, [c_void_p, c_int, c_int, c_int, c_void_p, c_int, c_int, c_int, c_int, c_void_p, c_void_p]),
    "gcv_frame_hist": (c_int, [c_void_p, c_int, c_int, c_int, c_int, c_void_p, c_void_p]),
    "gcv_hist_diff": (c_int, [c_void_p, c_int, c_int, c_void_p, c_void_p]),
    "gcv_frame_cells": (c_int, [c_void_p, c_int, c_int, c_int, c_int, c_void_p, c_void_p]),
    "gcv_blend_fit": (c_int, [c_void_p, c_int, c_int, c_int, c_void_p, c_void_p]),
    "gcv_hist_diff_lag": (c_int, [c_void_p, c_int, c_int, c_int, c_void_p, c_void_p]),
    "gcv_face_quality": (c_int, [c_void_p, c_int, c_int, c_int, c_void_p, c_int, c_int, c_void_p, c_void_p]),
    "gcv_face_signature": (c_int, [c_void_p, c_int, c_int, c_int, c_void_p, c_int, c_void_p, c_void_p]),
    "gcv_sig_link": (c_int, [c_void_p, c_void_p, c_int, c_int, c_void_p, c_void_p]),
    "gcv_vote_segments": (c_int, [c_void_p, c_int, c_int, c_void_p, c_int, c_void_p, c_void_p]),
    "gcv_vote_windows": (c_int, [c_void_p, c_int, c_int, c_void_p, c_int, c_void_p, c_void_p, c_void_p]),
    "gcv_tap_set": (c_int, [c_void_p, c_char_p, c_void_p, c_size_t]),
    "gcv_tap_clear": (c_int, [c_void_p]),
    "gcv_tap_written": (c_int, [c_void_p, c_char_p]),
    "gcv_profile_enable": (c_int, [c_void_p, c_int]),
    "gcv_profile_report": (c_char_p, [c_void_p]),
    "gcv_k_gemm": (c_int, [c_int, c_int, c_int, ctypes.POINTER(GemmArgs), c_void_p]),
    "gcv_gemm_plan": (c_int, [c_int, c_int, c_int, ctypes.POINTER(GemmArgs), c_void_p]),
    "gcv_k_stem_ln": (c_int, [c_int, c_void_p, c_int64, c_int64, c_int64, c_int64, c_void_p, c_void_p, c_void_p,
                              c_void_p, c_void_p, c_int, c_int, c_int, c_float, c_void_p]),
    "gcv_k_stem_ln_c": (c_int, [c_int, c_void_p, c_int64, c_int64, c_int64, c_int64, c_void_p, c_void_p, c_void_p,
                                c_void_p, c_void_p, c_int, c_int, c_int, c_int, c_float, c_void_p]),
    "gcv_k_dwconv7_ln": (c_int, [c_int, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_int, c_int,
                                 c_int, c_int, c_float, c_void_p]),
    "gcv_k_dwconv7_ln2": (c_int, [c_int, c_void_p, c_void_p, c_int, c_int, c_int, c_void_p, c_void_p, c_int, c_int, c_int,
                                  c_void_p, c_void_p, c_void_p, c_void_p, c_int, c_float, c_void_p]),
    "gcv_k_dwconv7_ln_planned": (c_int, [c_int, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_int, c_int,
                                         c_int, c_int, c_float, c_int, c_void_p]),
    "gcv_k_dwconv7_ln2_planned": (c_int, [c_int, c_void_p, c_void_p, c_int, c_int, c_int, c_void_p, c_void_p, c_int, c_int,
                                          c_int, c_void_p, c_void_p, c_void_p, c_void_p, c_int, c_float, c_int, c_int,
                                          c_void_p]),
    "gcv_dw_plan": (c_int, [c_int, c_int, c_int, c_int, c_int, c_int, c_void_p]),
    "gcv_dw_plan2": (c_int, [c_int, c_int, c_int, c_int, c_int, c_int, c_int, c_int, c_void_p]),
    "gcv_mlp_plan": (c_int, [c_int, c_int, c_int, c_int, c_void_p]),
    "gcv_convnext_res_ok": (c_int, [c_int, c_int]),
    "gcv_k_ln_patchify": (c_int, [c_int, c_void_p, c_void_p, c_void_p, c_void_p, c_int, c_int, c_int, c_int, c_float,
                                  c_void_p]),
    "gcv_k_layernorm_rows": (c_int, [c_int, c_void_p, c_void_p, c_void_p, c_void_p, c_int64, c_int, c_float, c_void_p]),
    "gcv_k_pool_ln": (c_int, [c_int, c_void_p, c_void_p, c_void_p, c_void_p, c_int, c_int, c_int, c_float, c_void_p]),
    "gcv_k_pool_ln_rows": (c_int, [c_int, c_void_p, c_void_p, c_void_p, c_void_p, c_int, c_int, c_int, c_float, c_int, c_int,
                                   c_int, c_void_p]),
    "gcv_k_conv3_first": (c_int, [c_int, c_void_p, c_int64, c_int64, c_int64, c_int64, c_void_p, c_void_p, c_void_p,
                                  c_int, c_int, c_int, c_int, c_int, c_void_p]),
    "gcv_k_convt2_small": (c_int, [c_int, c_void_p, c_void_p, c_void_p, c_void_p, c_int, c_int, c_int, c_int, c_void_p]),
    "gcv_k_reparam": (c_int, [c_int, c_void_p, c_int, c_void_p, c_void_p, c_void_p, c_void_p, c_int, c_int, c_void_p]),
    "gcv_k_head_tail": (c_int, [c_int, c_void_p, c_void_p, c_void_p, c_void_p, c_int, c_int, c_void_p]),
    "gcv_k_head_tail_splitk": (c_int, [c_int, c_void_p, c_int, c_void_p, c_int, c_void_p, c_void_p, c_void_p, c_int, c_int,
                                       c_void_p]),
    "gcv_k_resize_mse": (c_int, [c_int, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_int, c_void_p]),
    "gcv_k_swin_window_attn": (c_int, [c_int, c_void_p, c_void_p, c_void_p, c_int, c_int, c_int, c_int, c_int, c_int,
                                       c_void_p]),
    "gcv_k_patch_merge_ln": (c_int, [c_int, c_void_p, c_void_p, c_void_p, c_void_p, c_int, c_int, c_int, c_int, c_float,
                                     c_void_p]),
    "gcv_k_mean_tokens": (c_int, [c_int, c_void_p, c_void_p, c_int, c_int, c_int, c_void_p]),
    "gcv_k_head_bwd": (c_int, [c_int, c_void_p, c_int, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p,
                               c_int, c_int, c_void_p]),
    "gcv_k_bb_bwd": (c_int, [c_int, c_void_p, c_void_p, c_void_p, c_int, c_int, c_void_p]),
    "gcv_k_cam": (c_int, [c_int, c_int, c_int, c_void_p, c_void_p, c_int, c_int, c_int, c_int, c_int, c_int, c_void_p,
                          c_void_p, c_void_p, c_void_p, c_float, c_int, c_void_p]),
    "gcv_k_pool_ln_bwd": (c_int, [c_int, c_int, c_int, c_void_p, c_void_p, c_int, c_int, c_int, c_int, c_void_p, c_void_p,
                                  c_void_p, c_float, c_int, c_void_p]),
    "gcv_k_scale_rows": (c_int, [c_int, c_void_p, c_void_p, c_void_p, c_void_p, c_int, c_int, c_void_p]),
    "gcv_k_gelu_bwd": (c_int, [c_int, c_void_p, c_void_p, c_void_p, c_void_p, c_int, c_int, c_void_p]),
    "gcv_k_dw_ln_bwd": (c_int, [c_int, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_int, c_int,
                                c_int, c_float, c_void_p]),
    "gcv_k_dw_dgrad_res": (c_int, [c_void_p, c_void_p, c_void_p, c_int, c_int, c_int, c_void_p]),
    "gcv_k_down_ln_bwd": (c_int, [c_int, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_int, c_int, c_int, c_float,
                                  c_void_p]),
    "gcv_k_cam2": (c_int, [c_int, c_int, c_int, c_void_p, c_void_p, c_void_p, c_void_p, c_int, c_int, c_int, c_int, c_int,
                           c_int, c_void_p, c_void_p, c_void_p, c_int, c_void_p]),
    "gcv_k_fused_mlp": (c_int, [c_int, c_int, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p,
                                c_void_p, c_int, c_void_p]),
    "gcv_k_fused_mlp_lnp": (c_int, [c_int, c_int, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p,
                                    c_void_p, c_void_p, c_float, c_int, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p,
                                    c_int, c_void_p]),
    "gcv_k_fused_mlp_planned": (c_int, [c_int, c_int, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p,
                                        c_void_p, c_int, c_int, c_void_p]),
    "gcv_k_fused_mlp_lnp_planned": (c_int, [c_int, c_int, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p,
                                            c_void_p, c_void_p, c_void_p, c_float, c_int, c_void_p, c_void_p, c_void_p,
                                            c_void_p, c_void_p, c_int, c_int, c_void_p]),
    "gcv_k_fused_mlp_timed": (c_int, [c_int, c_int, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p,
                                      c_void_p, c_void_p, c_int, c_int, c_void_p, c_void_p]),
}

_lib = None
_lock = threading.Lock()


class GenConViTHipError(RuntimeError):
    pass


def _preload_hip_runtime():
    cands = []
    try:
        import torch
        cands.append(os.path.join(os.path.dirname(torch.__file__), "lib", "libamdhip64.so"))
    except Exception:   # torch not importable: plain C-ABI use
        pass
    cands += ["/opt/rocm/lib/libamdhip64.so", "libamdhip64.so"]
    last = None
    for c in cands:
        if os.path.isabs(c) and not os.path.exists(c):
            continue
        try:
            return ctypes.CDLL(c, mode=ctypes.RTLD_GLOBAL)
        except OSError as e:   # try the next candidate
            last = e
    raise GenConViTHipError(f"cannot load a HIP runtime (libamdhip64.so): {last}")


def load():
    """Load (once) and return the ctypes library with all signatures set.  Raises if absent."""
    global _lib
    with _lock:
        if _lib is not None:
            return _lib
        if not os.path.exists(LIB_PATH):
            raise GenConViTHipError(
                f"{LIB_PATH} not found — build it with `python -c 'import __graft_entry__ as g; g.build()'` "
                "(or `make -C genconvit_amd/csrc`). There is no CPU fallback.")
        _preload_hip_runtime()
        lib = ctypes.CDLL(LIB_PATH)
        for name, (res, args) in SIGNATURES.items():
            fn = getattr(lib, name)    # AttributeError if the symbol is not exported
            fn.restype = res
            fn.argtypes = args
        _lib = lib
        return lib


def last_error() -> str:
    return (load().gcv_last_error() or b"").decode(errors="replace")


def check(rc: int, what: str):
    if rc != 0:
        raise GenConViTHipError(f"{what} failed (rc={rc}): {last_error()}")


def dtype_code(torch_dtype) -> int:
    import torch
    try:
        return {torch.float32: GCV_F32, torch.bfloat16: GCV_BF16, torch.float16: GCV_F16}[torch_dtype]
    except KeyError:
        raise GenConViTHipError(f"unsupported dtype {torch_dtype}; use float32, bfloat16 or float16") from None


def current_stream_ptr(device) -> int:
    import torch
    return torch.cuda.current_stream(device).cuda_stream


# ConvNeXt backbone of a handle (include/genconvit_hip.h, GCV_CONVNEXT_*) and the largest max_batch each one takes
ARCH_TINY, ARCH_LARGE = 0, 1
ARCH_CODES = {"convnext_tiny": ARCH_TINY, "convnext_large": ARCH_LARGE}
ARCH_MAX_BATCH = {ARCH_TINY: 512, ARCH_LARGE: 256}


class Handle:
    """Owns one ``gcv_handle`` (packed weights + workspace) on one device / dtype / ConvNeXt backbone (``arch``:
    ``ARCH_TINY`` or ``ARCH_LARGE``)."""

    def __init__(self, device_index: int, torch_dtype, max_batch: int, arch: int = ARCH_TINY):
        import torch
        self.lib = load()
        if not torch.cuda.is_available():
            raise GenConViTHipError("no HIP device visible: the GenConViT HIP path needs an MI355X (gfx950); "
                                    "there is no CPU fallback")
        self.device_index = int(device_index)
        self.dtype = torch_dtype
        self.max_batch = int(max_batch)
        self._h = c_void_p()
        check(self.lib.gcv_create_arch(ctypes.byref(self._h), self.device_index, dtype_code(torch_dtype), self.max_batch,
                                       int(arch)), "gcv_create_arch")
        self.arch = self.lib.gcv_handle_arch(self._h)

    def close(self):
        if getattr(self, "_h", None) is not None and self._h:
            self.lib.gcv_destroy(self._h)
            self._h = c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:   # interpreter shutdown
            pass

    # -- weights ---------------------------------------------------------------------------
    @staticmethod
    def _descs(state_dict, skip_prefixes=()):
        import torch
        keep = []
        names = []
        for k, v in state_dict.items():
            if not torch.is_tensor(v) or not v.is_floating_point() or any(k.startswith(p) or p in k for p in skip_prefixes):
                continue
            t = v.detach()
            if t.dtype != torch.float32 or not t.is_contiguous():
                t = t.float().contiguous()
            keep.append(t)
            names.append(k.encode())
        arr = (TensorDesc * len(keep))()
        for i, (n, t) in enumerate(zip(names, keep)):
            arr[i] = TensorDesc(n, t.data_ptr(), t.numel(), 1 if t.is_cuda else 0)
        return arr, keep, names

    _OFF_PATH = ("embedder.", "patch_embed.", "encoder.fc1.", "encoder.fc2.", "fc3.", "num_batches_tracked")

    def _settle(self):
        """The library reads the tensors with synchronous copies / null-stream kernels: whatever stream produced them
        (a non-blocking ``.to()``, a cast on a side stream) must have finished first."""
        import torch
        torch.cuda.synchronize(self.device_index)

    def load_ed(self, state_dict):
        self._settle()
        arr, keep, _ = self._descs(state_dict, self._OFF_PATH)
        check(self.lib.gcv_load_ed(self._h, arr, len(keep)), "gcv_load_ed")

    def load_vae(self, state_dict, with_var=True):
        """``with_var=False`` leaves ``encoder.var`` (1.26 GB fp32, only read for the optional KL output) unpacked."""
        self._settle()
        arr, keep, _ = self._descs(state_dict, self._OFF_PATH + (() if with_var else ("encoder.var.",)))
        check(self.lib.gcv_load_vae(self._h, arr, len(keep)), "gcv_load_vae")

    def load_swin(self, state_dict, prefix=""):
        self._settle()
        arr, keep, _ = self._descs(state_dict)
        check(self.lib.gcv_load_swin(self._h, arr, len(keep), prefix.encode()), "gcv_load_swin")

    # -- taps (tests: include/genconvit_hip.h, gcv_tap_set) ------------------------------------
    def set_tap(self, name, tensor):
        """Copy intermediate ``name`` into ``tensor`` (a contiguous device tensor of its exact size) at every following
        forward of this handle; ``tensor=None`` removes the tap.  The handle keeps a reference to the tensor."""
        taps = self.__dict__.setdefault("_taps", {})
        if tensor is None:
            check(self.lib.gcv_tap_set(self._h, name.encode(), None, 0), "gcv_tap_set")
            taps.pop(name, None)
            return
        if not (tensor.is_cuda and tensor.is_contiguous()):
            raise GenConViTHipError("a tap buffer must be a contiguous device tensor")
        check(self.lib.gcv_tap_set(self._h, name.encode(), tensor.data_ptr(), tensor.numel() * tensor.element_size()),
              "gcv_tap_set")
        taps[name] = tensor

    def clear_taps(self):
        check(self.lib.gcv_tap_clear(self._h), "gcv_tap_clear")
        self.__dict__.pop("_taps", None)

    def tap_written(self, name) -> bool:
        """True if the last forward stored all of tap ``name``; False if its dispatch never stores that tensor."""
        rc = self.lib.gcv_tap_written(self._h, name.encode())
        if rc < 0:
            check(rc, "gcv_tap_written")
        return rc == 1

    # -- forwards --------------------------------------------------------------------------
    def _check_x(self, x, res=224):
        import torch
        if not (torch.is_tensor(x) and x.is_cuda and x.device.index == self.device_index):
            raise GenConViTHipError(f"input must be a CUDA(HIP) tensor on device {self.device_index}")
        if x.dim() != 4 or x.shape[1] != 3 or x.shape[2] != res or x.shape[3] != res:
            raise GenConViTHipError(f"input must be (B,3,{res},{res}), got {tuple(x.shape)}")
        if x.dtype != self.dtype:
            raise GenConViTHipError(f"input dtype {x.dtype} != handle dtype {self.dtype}")
        if x.shape[0] < 1 or x.shape[0] > self.max_batch:
            raise GenConViTHipError(f"batch {x.shape[0]} outside [1,{self.max_batch}]")
        return x.contiguous()

    def ed_forward(self, x):
        import torch
        x = self._check_x(x)
        out = torch.empty((x.shape[0], 2), dtype=torch.float32, device=x.device)
        check(self.lib.gcv_ed_forward(self._h, x.data_ptr(), x.shape[0], out.data_ptr(), current_stream_ptr(x.device)),
              "gcv_ed_forward")
        return out

    def vae_forward(self, x, eps, want_recon=True, want_mse=False, want_kl=False):
        import torch
        x = self._check_x(x)
        B = x.shape[0]
        if not (torch.is_tensor(eps) and eps.is_cuda and eps.device.index == self.device_index and tuple(eps.shape) == (B, 12544)):
            raise GenConViTHipError(f"eps must be a tensor of shape ({B},12544) on device {self.device_index}")
        eps = eps.float().contiguous()
        out = torch.empty((B, 2), dtype=torch.float32, device=x.device)
        recon = torch.empty((B, 3, 224, 224), dtype=self.dtype, device=x.device) if want_recon else None
        mse = torch.empty((B,), dtype=torch.float32, device=x.device) if want_mse else None
        kl = torch.empty((1,), dtype=torch.float32, device=x.device) if want_kl else None
        p = lambda t: t.data_ptr() if t is not None else None
        check(self.lib.gcv_vae_forward(self._h, x.data_ptr(), eps.data_ptr(), B, out.data_ptr(), p(recon), p(mse), p(kl),
                                       current_stream_ptr(x.device)), "gcv_vae_forward")
        return out, recon, mse, kl

    # -- explain: Grad-CAM maps of the real / fake decision (include/genconvit_hip.h, gcv_*_explain) ---------------
    def _target(self, target, B, device):
        import torch
        if target is None:
            return None
        t = torch.as_tensor(target, device=device).to(torch.int32).reshape(-1).contiguous()
        if t.numel() == 1 and B != 1:
            t = t.expand(B).contiguous()
        if t.numel() != B:
            raise GenConViTHipError(f"target must hold one class per frame ({B}), got {t.numel()}")
        return t

    def ed_explain(self, x, target=None, upsample=True, layer="s3"):
        """ED forward + Grad-CAM.  Returns (logits (B,2), cam (B,2,7,7) fp32 [reconstruction pass, original pass] — (B,2,14,14)
        at ``layer`` "s2" —, cam224 (B,224,224) of the original pass or None).  ``layer``: see ``explain_layer``."""
        import torch
        x = self._check_x(x)
        B = x.shape[0]
        t = self._target(target, B, x.device)
        n, at = explain_layer(layer)
        side = 7 if n == 3 else 14
        out = torch.empty((B, 2), dtype=torch.float32, device=x.device)
        cam = torch.empty((B, 2, side, side), dtype=torch.float32, device=x.device)
        up = torch.empty((B, 224, 224), dtype=torch.float32, device=x.device) if upsample else None
        tp, upp = t.data_ptr() if t is not None else None, up.data_ptr() if up is not None else None
        if at:
            check(self.lib.gcv_ed_explain_at(self._h, x.data_ptr(), B, tp, n, out.data_ptr(), cam.data_ptr(), upp,
                                             current_stream_ptr(x.device)), "gcv_ed_explain_at")
        else:
            check(self.lib.gcv_ed_explain(self._h, x.data_ptr(), B, tp, out.data_ptr(), cam.data_ptr(), upp,
                                          current_stream_ptr(x.device)), "gcv_ed_explain")
        return out, cam, up

    def vae_explain(self, x, eps, target=None, upsample=True, layer="s3"):
        """VAE forward + Grad-CAM.  Returns (logits (B,2), cam (B,58) fp32 = [7x7 of x at 224 px, 3x3 of x_hat at 112 px] —
        (B,245) = [14x14, 7x7] at ``layer`` "s2" —, cam224 (B,224,224) of x or None).  ``layer``: see ``explain_layer``."""
        import torch
        x = self._check_x(x)
        B = x.shape[0]
        eps = self._check_eps(eps, B)
        t = self._target(target, B, x.device)
        n, at = explain_layer(layer)
        out = torch.empty((B, 2), dtype=torch.float32, device=x.device)
        cam = torch.empty((B, 58 if n == 3 else 245), dtype=torch.float32, device=x.device)
        up = torch.empty((B, 224, 224), dtype=torch.float32, device=x.device) if upsample else None
        tp, upp = t.data_ptr() if t is not None else None, up.data_ptr() if up is not None else None
        if at:
            check(self.lib.gcv_vae_explain_at(self._h, x.data_ptr(), eps.data_ptr(), B, tp, n, out.data_ptr(), cam.data_ptr(),
                                              upp, current_stream_ptr(x.device)), "gcv_vae_explain_at")
        else:
            check(self.lib.gcv_vae_explain(self._h, x.data_ptr(), eps.data_ptr(), B, tp, out.data_ptr(), cam.data_ptr(), upp,
                                           current_stream_ptr(x.device)), "gcv_vae_explain")
        return out, cam, up

    def _check_eps(self, eps, B):
        import torch
        if not (torch.is_tensor(eps) and eps.is_cuda and eps.device.index == self.device_index and tuple(eps.shape) == (B, 12544)):
            raise GenConViTHipError(f"eps must be a tensor of shape ({B},12544) on device {self.device_index}")
        return eps.float().contiguous()

    def convnext_forward(self, which, x):
        import torch
        x = self._check_x(x, res=x.shape[-1])
        out = torch.empty((x.shape[0], 1000), dtype=self.dtype, device=x.device)
        check(self.lib.gcv_convnext_forward(self._h, which, x.data_ptr(), x.shape[0], x.shape[-1], out.data_ptr(),
                                            current_stream_ptr(x.device)), "gcv_convnext_forward")
        return out

    def swin_forward(self, x):
        import torch
        x = self._check_x(x)
        out = torch.empty((x.shape[0], 1000), dtype=self.dtype, device=x.device)
        check(self.lib.gcv_swin_forward(self._h, x.data_ptr(), x.shape[0], out.data_ptr(), current_stream_ptr(x.device)),
              "gcv_swin_forward")
        return out

    def workspace_bytes(self) -> int:
        return int(self.lib.gcv_workspace_bytes(self._h))

    def profile_enable(self, on=True):
        check(self.lib.gcv_profile_enable(self._h, 1 if on else 0), "gcv_profile_enable")

    def profile_report(self):
        return json.loads((self.lib.gcv_profile_report(self._h) or b"[]").decode())


def genconvit_forward(h_ed: "Handle", h_vae: "Handle", x, eps):
    """``GenConViT.forward`` for net='genconvit' (model/genconvit.py:66-75) through ``gcv_genconvit_forward``: ED and VAE
    on two streams inside the library, joined back into the current stream; returns the (2B,2) fp32 logits."""
    import torch
    x = h_ed._check_x(x)
    B = x.shape[0]
    if h_vae.device_index != h_ed.device_index or h_vae.dtype != h_ed.dtype:
        raise GenConViTHipError("ED and VAE handles must share device and dtype")
    if not (torch.is_tensor(eps) and eps.is_cuda and eps.device.index == h_ed.device_index and tuple(eps.shape) == (B, 12544)):
        raise GenConViTHipError(f"eps must be a tensor of shape ({B},12544) on device {h_ed.device_index}")
    eps = eps.float().contiguous()
    out = torch.empty((2 * B, 2), dtype=torch.float32, device=x.device)
    check(h_ed.lib.gcv_genconvit_forward(h_ed._h, h_vae._h, x.data_ptr(), eps.data_ptr(), B, out.data_ptr(),
                                         current_stream_ptr(x.device)), "gcv_genconvit_forward")
    return out


EXPLAIN_LAYERS = {"s3": 3, "s2": 2}


def explain_layer(layer):
    """The ConvNeXt stage an explain call takes its maps at, as (stage number, whether the call goes through
    ``gcv_*_explain_at``).  "s3" (the default): the last stage, through ``gcv_*_explain``; "s2": the output of stage 2,
    14 x 14 cells; the integers 3 / 2 name the same stages and always go through ``gcv_*_explain_at``."""
    if isinstance(layer, str) and layer in EXPLAIN_LAYERS:
        return EXPLAIN_LAYERS[layer], layer != "s3"
    if isinstance(layer, int) and not isinstance(layer, bool) and layer in (2, 3):
        return layer, True
    raise ValueError(f"unknown explain layer {layer!r}: accepted values are 's3' and 's2'")


def genconvit_explain(h_ed: "Handle", h_vae: "Handle", x, eps, target=None, upsample=True, layer="s3"):
    """``genconvit_forward`` + Grad-CAM of both networks (``gcv_genconvit_explain``).  Returns (logits (2B,2),
    cam_ed (B,2,7,7), cam_vae (B,58), cam224 (2B,224,224) or None) — cam224 rows in the logits' row order.  At ``layer``
    "s2" (``explain_layer``): cam_ed (B,2,14,14), cam_vae (B,245)."""
    import torch
    x = h_ed._check_x(x)
    B = x.shape[0]
    if h_vae.device_index != h_ed.device_index or h_vae.dtype != h_ed.dtype:
        raise GenConViTHipError("ED and VAE handles must share device and dtype")
    eps = h_ed._check_eps(eps, B)
    t = h_ed._target(target, B, x.device)
    out = torch.empty((2 * B, 2), dtype=torch.float32, device=x.device)
    n, at = explain_layer(layer)
    side, ne, nv = (7, 98, 58) if n == 3 else (14, 392, 245)
    cam = torch.empty((B * (ne + nv),), dtype=torch.float32, device=x.device)
    up = torch.empty((2 * B, 224, 224), dtype=torch.float32, device=x.device) if upsample else None
    tp, upp = t.data_ptr() if t is not None else None, up.data_ptr() if up is not None else None
    if at:
        check(h_ed.lib.gcv_genconvit_explain_at(h_ed._h, h_vae._h, x.data_ptr(), eps.data_ptr(), B, tp, n, out.data_ptr(),
                                                cam.data_ptr(), upp, current_stream_ptr(x.device)),
              "gcv_genconvit_explain_at")
    else:
        check(h_ed.lib.gcv_genconvit_explain(h_ed._h, h_vae._h, x.data_ptr(), eps.data_ptr(), B, tp, out.data_ptr(),
                                             cam.data_ptr(), upp, current_stream_ptr(x.device)), "gcv_genconvit_explain")
    return out, cam[:B * ne].view(B, 2, side, side), cam[B * ne:].view(B, nv), up


class Comm:
    """RCCL communicator of the C ABI (``gcv_comm_*``): one per process group, used for the logit all-gather."""

    @staticmethod
    def _share_torch_rccl():
        """Every rank must bind the SAME RCCL build (the one torch.distributed already uses in this process): point the
        library's run-time loader at torch's bundled copy unless the caller chose one."""
        try:
            import torch
            path = os.path.join(os.path.dirname(torch.__file__), "lib", "librccl.so")
            if os.path.exists(path):
                os.environ.setdefault("GCV_RCCL_PATH", path)
        except Exception:
            pass

    def __init__(self, world: int, rank: int, unique_id: bytes, device_index: int):
        self._share_torch_rccl()
        self.lib = load()
        self.world, self.rank, self.device_index = int(world), int(rank), int(device_index)
        self._c = c_void_p()
        buf = ctypes.create_string_buffer(bytes(unique_id), 128)
        check(self.lib.gcv_comm_create(ctypes.byref(self._c), self.world, self.rank, buf, self.device_index), "gcv_comm_create")

    @staticmethod
    def available() -> bool:
        """RCCL and its entry points can be bound in this process (dlopen + dlsym; starts nothing)."""
        Comm._share_torch_rccl()
        return bool(load().gcv_comm_available())

    def count(self) -> int:
        """Ranks in the communicator as RCCL itself reports them (ncclCommCount)."""
        return int(self.lib.gcv_comm_count(self._c))

    @staticmethod
    def unique_id() -> bytes:
        Comm._share_torch_rccl()
        buf = ctypes.create_string_buffer(128)
        check(load().gcv_comm_unique_id(buf), "gcv_comm_unique_id")
        return buf.raw

    def allgather(self, local):
        """local: fp32 device tensor (same numel on every rank) -> (world, *local.shape)."""
        import torch
        local = local.float().contiguous()
        out = torch.empty((self.world,) + tuple(local.shape), dtype=torch.float32, device=local.device)
        check(self.lib.gcv_allgather_logits(self._c, local.data_ptr(), local.numel(), out.data_ptr(),
                                            current_stream_ptr(local.device)), "gcv_allgather_logits")
        return out

    def close(self):
        if getattr(self, "_c", None) is not None and self._c:
            self.lib.gcv_comm_destroy(self._c)
            self._c = c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def _check_frames(frames_u8, expects, least=0, on_device=True):
    """``frames_u8`` as a contiguous uint8 (F,H,W,3) tensor, F >= ``least``, on a device unless ``on_device`` is False (the
    caller then looks at the device itself), and (F, H, W); anything else is an error that says ``expects``."""
    import torch
    if not (torch.is_tensor(frames_u8) and (frames_u8.is_cuda or not on_device) and frames_u8.dtype == torch.uint8
            and frames_u8.dim() == 4 and frames_u8.shape[3] == 3 and frames_u8.shape[0] >= least):
        raise GenConViTHipError(expects)
    return frames_u8.contiguous(), tuple(int(v) for v in frames_u8.shape[:3])


def preprocess(frames_u8, dtype=None):
    """Device-side ``preprocess_frame`` (model/pred_func.py:95-108): uint8 (N,H,W,3) device tensor ->
    normalised (N,3,H,W) tensor of ``dtype`` (fp32 by default, like the reference)."""
    import torch
    dtype = dtype or torch.float32
    frames_u8, (n, h, w) = _check_frames(frames_u8, "preprocess expects a uint8 device tensor of shape (N,H,W,3)")
    code = dtype_code(dtype)
    out = torch.empty((n, 3, h, w), dtype=dtype, device=frames_u8.device)
    check(load().gcv_preprocess(code, frames_u8.data_ptr(), out.data_ptr(), n, h, w, current_stream_ptr(frames_u8.device)),
          "gcv_preprocess")
    return out


def face_crop_resize(frames_u8, boxes, size=224):
    """Row N4: ``cv2.resize(frame[top:bottom, left:right], (size, size), interpolation=cv2.INTER_AREA)`` of face_rec
    (model/pred_func.py:79-85) for all boxes in one launch.  ``frames_u8``: (F,H,W,3) uint8 device tensor (RGB);
    ``boxes``: (n,5) integers (frame index, top, right, bottom, left).  Returns (n,size,size,3) uint8 on the device.
    Boxes outside their frame are an error here (the kernel itself would write zeros for them)."""
    import torch
    frames_u8, (nf, h, w) = _check_frames(frames_u8, "face_crop_resize expects a uint8 device tensor of shape (F,H,W,3)")
    b = _check_boxes("face_crop_resize", boxes, nf, h, w)
    lib = load()
    out = torch.empty((b.shape[0], size, size, 3), dtype=torch.uint8, device=frames_u8.device)
    if b.shape[0] == 0:
        return out
    bd = b.to(frames_u8.device)
    check(lib.gcv_face_crop_resize(frames_u8.data_ptr(), nf, h, w, bd.data_ptr(), b.shape[0], out.data_ptr(), size,
                                   current_stream_ptr(frames_u8.device)), "gcv_face_crop_resize")
    return out


def face_crop_preprocess(frames_u8, boxes, size=224, dtype=None):
    """``preprocess(face_crop_resize(frames_u8, boxes, size), dtype)`` in one launch (``gcv_face_crop_preprocess``), bit for
    bit: the boxes of the (F,H,W,3) uint8 device frames go straight to the network's normalised (n,3,size,size) input of
    ``dtype`` (fp32 by default) with no uint8 image in between.  Boxes as for ``face_crop_resize``: one outside its frame
    is an error, none give an empty tensor."""
    import torch
    dtype = dtype or torch.float32
    frames_u8, (nf, h, w) = _check_frames(frames_u8, "face_crop_preprocess expects a uint8 device tensor of shape (F,H,W,3)")
    b = _check_boxes("face_crop_preprocess", boxes, nf, h, w)
    code = dtype_code(dtype)
    lib = load()
    out = torch.empty((b.shape[0], 3, size, size), dtype=dtype, device=frames_u8.device)
    if b.shape[0] == 0:
        return out
    bd = b.to(frames_u8.device)
    check(lib.gcv_face_crop_preprocess(code, frames_u8.data_ptr(), nf, h, w, bd.data_ptr(), b.shape[0], out.data_ptr(),
                                       size, current_stream_ptr(frames_u8.device)), "gcv_face_crop_preprocess")
    return out


def _check_boxes(what, boxes, nf, h, w):
    """``boxes`` as an (n,5) int32 host tensor; a box outside its (h, w) frame is an error."""
    import torch
    b = torch.as_tensor(boxes, dtype=torch.int32).reshape(-1, 5).cpu()
    if b.numel():
        f, top, right, bottom, left = b.unbind(1)
        ok = (f >= 0) & (f < nf) & (top >= 0) & (left >= 0) & (bottom <= h) & (right <= w) & (top < bottom) & (left < right)
        if not bool(ok.all()):
            raise GenConViTHipError(f"{what}: box {int((~ok).nonzero()[0])} lies outside its {h}x{w} frame")
    return b


TRACK_GRIDS, TRACK_RADIUS_MAX, TRACK_WEIGHT_MAX = (16, 32, 64), 32, 1024


def _check_track_jobs(what, jobs, nf, h, w, grid):
    """``jobs`` as an (n,17) int32 host tensor (``gcv_track_match``, include/genconvit_hip.h); a frame index out of range, a
    box outside its (h, w) frame or smaller than ``grid`` a side, or weights outside wa, wb >= 0, 1 <= wa + wb <= 1024 is
    an error."""
    import torch
    j = torch.as_tensor(jobs, dtype=torch.int32).reshape(-1, 17).cpu()
    if j.numel():
        ok = torch.ones(j.shape[0], dtype=torch.bool)
        for c in (0, 5, 11):
            f, top, right, bottom, left = j[:, c:c + 5].unbind(1)
            ok &= (f >= 0) & (f < nf) & (top >= 0) & (left >= 0) & (bottom <= h) & (right <= w)
            ok &= (bottom.long() - top.long() >= grid) & (right.long() - left.long() >= grid)
        wa, wb = j[:, 10].long(), j[:, 16].long()
        ok &= (wa >= 0) & (wb >= 0) & (wa + wb >= 1) & (wa + wb <= TRACK_WEIGHT_MAX)
        if not bool(ok.all()):
            raise GenConViTHipError(f"{what}: job {int((~ok).nonzero()[0])} has a frame index out of range, a box outside its "
                                    f"{h}x{w} frame or smaller than {grid} a side, or weights outside 1 <= wa + wb <= "
                                    f"{TRACK_WEIGHT_MAX}")
    return j


def _check_grid_radius(what, grid, radius):
    """(grid, radius) as integers; a grid outside ``TRACK_GRIDS`` and a radius outside 0 ... ``TRACK_RADIUS_MAX`` are errors."""
    grid, radius = int(grid), int(radius)
    if grid not in TRACK_GRIDS:
        raise GenConViTHipError(f"{what}: grid {grid}; accepted values are 16, 32 and 64")
    if not 0 <= radius <= TRACK_RADIUS_MAX:
        raise GenConViTHipError(f"{what}: radius {radius} outside 0 ... {TRACK_RADIUS_MAX}")
    return grid, radius


def track_match(frames_u8, jobs, grid=64, radius=16):
    """Where is the face in a frame the detector skipped (``gcv_track_match``, include/genconvit_hip.h: the arithmetic is
    stated there): integer block matching on a ``grid`` x ``grid`` lattice of mean-luma cells, searched ``radius`` cells
    either way around the prior box, against the two detections around the gap.  ``frames_u8``: (F,H,W,3) uint8 device
    tensor (RGB); ``jobs``: (n,17) integers, per row (fs, top, right, bottom, left) the skipped frame and the prior box,
    (fa, ta, ra, ba, la, wa) and (fb, tb, rb, bb, lb, wb) the two anchors and their weights.  Returns (n,4) int32 on the
    device: (oy, ox, best cost, cost at zero displacement) with (oy, ox) the pixel offset to add to the prior box.  A
    ``grid`` other than 16, 32, 64, a ``radius`` outside 0 ... 32 and a bad row are errors; none give an empty tensor."""
    import torch
    frames_u8, (nf, h, w) = _check_frames(frames_u8, "track_match expects a uint8 device tensor of shape (F,H,W,3)")
    grid, radius = _check_grid_radius("track_match", grid, radius)
    j = _check_track_jobs("track_match", jobs, nf, h, w, grid)
    lib = load()
    n = j.shape[0]
    out = torch.empty((n, 4), dtype=torch.int32, device=frames_u8.device)
    if n == 0:
        return out
    jd = j.contiguous().to(frames_u8.device)
    check(lib.gcv_track_match(frames_u8.data_ptr(), nf, h, w, jd.data_ptr(), n, grid, radius, out.data_ptr(),
                              current_stream_ptr(frames_u8.device)), "gcv_track_match")
    return out


TRACK_CHAIN_STEPS_MAX, TRACK_CHAIN_NONE = 1024, (0, 0, -1, -1)


def _check_chain_jobs(what, jobs, nf, h, w, grid):
    """``jobs`` as an (n,11) int32 host tensor (``gcv_track_chain``, include/genconvit_hip.h); a frame index of the template
    or of any step out of range, a template box or first prior box outside its (h, w) frame, a template lower or narrower
    than ``grid``, a ``dir`` other than +-1, ``steps`` outside 1 ... 1024 and a negative ``stop`` are errors."""
    import torch
    j = torch.as_tensor(jobs, dtype=torch.int32).reshape(-1, 11).cpu()
    if j.numel():
        fa, top, right, bottom, left, fs, step, steps, py, px, stop = j.long().unbind(1)
        last = fs + step * (steps - 1)
        ok = (fa >= 0) & (fa < nf) & (top >= 0) & (left >= 0) & (bottom <= h) & (right <= w)
        ok &= (bottom - top >= grid) & (right - left >= grid) & (step.abs() == 1)
        ok &= (steps >= 1) & (steps <= TRACK_CHAIN_STEPS_MAX) & (fs >= 0) & (fs < nf) & (last >= 0) & (last < nf)
        ok &= (top + py >= 0) & (bottom + py <= h) & (left + px >= 0) & (right + px <= w) & (stop >= 0)
        if not bool(ok.all()):
            raise GenConViTHipError(f"{what}: job {int((~ok).nonzero()[0])} has a frame index out of range, a template or "
                                    f"first prior box outside its {h}x{w} frame or smaller than {grid} a side, a dir other "
                                    f"than +-1, steps outside 1 ... {TRACK_CHAIN_STEPS_MAX} or a negative stop")
    return j


def track_chain(frames_u8, jobs, grid=64, radius=8):
    """Where does the face go before its first or after its last detection (``gcv_track_chain``, include/genconvit_hip.h:
    the arithmetic is stated there): ``track_match``'s search walked along consecutive frames, every step around the box the
    step before found, against one template that is not updated.  ``frames_u8``: (F,H,W,3) uint8 device tensor (RGB);
    ``jobs``: (n,11) integers, per row (fa, top, right, bottom, left) the template, (fs, dir, steps) the frames fs, fs + dir,
    ..., (py, px) the offset of the first prior box from the template box and ``stop`` the cost above which the chain ends.
    Returns (n, max(steps), 4) int32 on the device: per step (oy, ox, best cost, cost at zero displacement) with (oy, ox)
    relative to that step's prior, and (0, 0, -1, -1) from the step that exceeded ``stop``, and from ``steps``, on.  A ``grid``
    other than 16, 32, 64, a ``radius`` outside 0 ... 32 and a bad row are errors; no rows give an empty (0, 0, 4) tensor."""
    import torch
    frames_u8, (nf, h, w) = _check_frames(frames_u8, "track_chain expects a uint8 device tensor of shape (F,H,W,3)")
    grid, radius = _check_grid_radius("track_chain", grid, radius)
    j = _check_chain_jobs("track_chain", jobs, nf, h, w, grid)
    lib = load()
    n = j.shape[0]
    if n == 0:
        return torch.empty((0, 0, 4), dtype=torch.int32, device=frames_u8.device)
    max_steps = int(j[:, 7].max())
    out = torch.empty((n, max_steps, 4), dtype=torch.int32, device=frames_u8.device)
    jd = j.contiguous().to(frames_u8.device)
    check(lib.gcv_track_chain(frames_u8.data_ptr(), nf, h, w, jd.data_ptr(), n, max_steps, grid, radius, out.data_ptr(),
                              current_stream_ptr(frames_u8.device)), "gcv_track_chain")
    return out


def face_quality(frames_u8, boxes, grid=64):
    """Is a face crop usable (``gcv_face_quality``, include/genconvit_hip.h: the arithmetic is stated there): sums over a
    ``grid`` x ``grid`` lattice of mean-luma cells of every box, all boxes in one launch.  ``frames_u8``: (F,H,W,3) uint8
    device tensor (RGB); a slice such as ``frames[1:]`` is used in place, whatever its alignment.  ``boxes``: (n,5) integers
    (frame index, top, right, bottom, left).  Returns (n,8) int64 on the device: (G, S1, S2, L2, GX, GY, dark, bright) — the
    sum and the sum of squares of the cells, the energy of their Laplacian and of their differences along the rows and
    down the columns, and the number of cells below 16 and above 239.  A ``grid`` other than 16, 32, 64, a box outside its
    frame and a box lower or narrower than ``grid`` are errors here, before anything is launched (the zeros row is the C
    entry's guard); none give an empty tensor."""
    import torch
    grid = int(grid)
    if grid not in TRACK_GRIDS:
        raise GenConViTHipError(f"face_quality: grid {grid}; accepted values are 16, 32 and 64")
    frames_u8, (nf, h, w) = _check_frames(frames_u8, "face_quality expects a uint8 device tensor of shape (F,H,W,3)")
    b = _check_quality_boxes("face_quality", boxes, nf, h, w, grid)
    lib = load()
    n = b.shape[0]
    out = torch.empty((n, 8), dtype=torch.int64, device=frames_u8.device)
    if n == 0:
        return out
    bd = b.contiguous().to(frames_u8.device)
    check(lib.gcv_face_quality(frames_u8.data_ptr(), nf, h, w, bd.data_ptr(), n, grid, out.data_ptr(),
                               current_stream_ptr(frames_u8.device)), "gcv_face_quality")
    return out


def _check_quality_boxes(what, boxes, nf, h, w, grid):
    """``_check_boxes``, and a box lower or narrower than ``grid`` is an error too."""
    b = _check_boxes(what, boxes, nf, h, w)
    if b.numel():
        small = ((b[:, 3] - b[:, 1]) < grid) | ((b[:, 2] - b[:, 4]) < grid)
        if bool(small.any()):
            raise GenConViTHipError(f"{what}: box {int(small.nonzero()[0])} is smaller than grid = {grid} a side")
    return b


SIG_GRID, SIG_BYTES, SIG_MAX_ROWS, SIG_MAX_TRACKS, SIG_NONE = 16, 384, 65536, 4096, 0xFFFFFFFF


def face_signature(frames_u8, boxes):
    """What does a face crop look like (``gcv_face_signature``, include/genconvit_hip.h: the arithmetic is stated there): per
    box 384 bytes — the mean-luma cells of a 16 x 16 grid with the box's own mean and spread taken out, then Cb and Cr on
    an 8 x 8 grid — all boxes in one launch.  ``frames_u8``: (F,H,W,3) uint8 device tensor (RGB); a slice such as
    ``frames[1:]`` is used in place, whatever its alignment.  ``boxes``: (n,5) integers (frame index, top, right, bottom,
    left).  Returns (n,384) uint8 on the device.  A box outside its frame and a box lower or narrower than 16 pixels are
    errors here, before anything is launched (the zeros row is the C entry's guard); none give an empty tensor."""
    import torch
    frames_u8, (nf, h, w) = _check_frames(frames_u8, "face_signature expects a uint8 device tensor of shape (F,H,W,3)")
    b = _check_quality_boxes("face_signature", boxes, nf, h, w, SIG_GRID)
    lib = load()
    n = b.shape[0]
    out = torch.empty((n, SIG_BYTES), dtype=torch.uint8, device=frames_u8.device)
    if n == 0:
        return out
    bd = b.contiguous().to(frames_u8.device)
    check(lib.gcv_face_signature(frames_u8.data_ptr(), nf, h, w, bd.data_ptr(), n, out.data_ptr(),
                                 current_stream_ptr(frames_u8.device)), "gcv_face_signature")
    return out


def _check_sig_link(what, sig, owner, tracks):
    """``owner`` as an (n,) int32 host tensor and ``tracks`` as an int; the shapes, the limits of ``gcv_sig_link`` and an
    owner outside [-1, tracks) are errors."""
    import torch
    if not (torch.is_tensor(sig) and sig.dtype == torch.uint8 and sig.dim() == 2 and sig.shape[1] == SIG_BYTES):
        raise GenConViTHipError(f"{what} expects the signatures as a uint8 tensor of shape (n,{SIG_BYTES})")
    if isinstance(tracks, bool) or int(tracks) != tracks or not 0 <= int(tracks) <= SIG_MAX_TRACKS:
        raise GenConViTHipError(f"{what}: tracks {tracks} outside 0 ... {SIG_MAX_TRACKS}")
    tracks = int(tracks)
    o = torch.as_tensor(owner, dtype=torch.int32).reshape(-1).cpu()
    n = sig.shape[0]
    if o.numel() != n:
        raise GenConViTHipError(f"{what}: {o.numel()} owners for {n} signatures")
    if n > SIG_MAX_ROWS:
        raise GenConViTHipError(f"{what}: {n} signatures; at most {SIG_MAX_ROWS} go into one call")
    if n and not bool(((o >= -1) & (o < tracks)).all()):
        bad = int(((o < -1) | (o >= tracks)).nonzero()[0])
        raise GenConViTHipError(f"{what}: owner {int(o[bad])} of row {bad} is neither -1 nor a track in [0, {tracks})")
    return o, tracks


def sig_link(sig, owner, tracks):
    """How alike are two tracks at their best (``gcv_sig_link``, include/genconvit_hip.h): ``out[a][b]``, a != b, is the
    smallest L1 distance between a signature of track a and one of track b, over all such pairs of rows.  ``sig``: (n,384)
    uint8 device tensor (``face_signature``); ``owner``: n integers, the track of each row in [0, ``tracks``) or -1 for a
    row that takes no part, in any order; ``tracks``: T.  Returns (T,T) int64 on the device — torch has no arithmetic on
    uint32, and int64 holds the C entry's 0xFFFFFFFF (``SIG_NONE``: the diagonal, and every pair one of whose tracks has no
    row) as itself; every other value is at most 384 * 255 = 97 920.  More than 65 536 rows or 4 096 tracks, an owner
    outside [-1, T), a host tensor and a wrong shape are errors here, before anything is launched; no row or T = 0
    launches nothing."""
    import torch
    o, tracks = _check_sig_link("sig_link", sig, owner, tracks)
    if not sig.is_cuda:
        raise GenConViTHipError("sig_link expects the signatures as a device tensor")
    lib = load()
    n = sig.shape[0]
    if n == 0 or tracks == 0:
        return torch.full((tracks, tracks), SIG_NONE, dtype=torch.int64, device=sig.device)
    sig = sig.contiguous()
    if sig.data_ptr() % 16:
        sig = sig.clone()                                   # a view that starts inside an allocation, off a 16-byte boundary
    od = o.contiguous().to(sig.device)
    out = torch.empty((tracks, tracks), dtype=torch.int32, device=sig.device)       # the C entry's uint32, bit for bit
    check(lib.gcv_sig_link(sig.data_ptr(), od.data_ptr(), n, tracks, out.data_ptr(), current_stream_ptr(sig.device)),
          "gcv_sig_link")
    return out.to(torch.int64) & SIG_NONE


CUT_REGIONS, CUT_BINS = (1, 2, 4, 8), 64


def _out_buffer(what, out, shape, device, dtype=None):
    """``out`` if it is a contiguous tensor of ``dtype`` (int32 by default) and ``shape`` on ``device``, a new one for None,
    else an error."""
    import torch
    dtype = dtype or torch.int32
    if out is None:
        return torch.empty(shape, dtype=dtype, device=device)
    if not (torch.is_tensor(out) and out.dtype == dtype and out.device == device and tuple(out.shape) == shape
            and out.is_contiguous()):
        raise GenConViTHipError(f"{what}: out must be a contiguous {str(dtype).replace('torch.', '')} tensor of shape {shape} "
                                f"on {device}")
    return out


def frame_hist(frames_u8, regions=4, out=None):
    """Luma histograms of the ``regions`` x ``regions`` parts of every frame (``gcv_frame_hist``, include/genconvit_hip.h: the
    arithmetic is stated there).  ``frames_u8``: (F,H,W,3) uint8 device tensor (RGB), F >= 1; a slice such as ``frames[1:]``
    is used in place, whatever its alignment.  Returns (F, regions^2, 64) int32 on the device: the C entry's uint32 counts,
    which stay below 2^31 (a frame holds at most 2^30 pixels).  ``out``: write into this contiguous int32 tensor of that
    shape on the same device instead of a new one (the rows of one group of frames in a whole video's buffer).  ``regions``
    other than 1, 2, 4, 8, a frame lower or narrower than ``regions``, more than 2^30 pixels a frame, a host tensor and a
    wrong shape or dtype are errors."""
    frames_u8, (nf, h, w) = _check_frames(frames_u8, "frame_hist expects a uint8 device tensor of shape (F,H,W,3), F >= 1", 1)
    if isinstance(regions, bool) or not isinstance(regions, int) or regions not in CUT_REGIONS:
        raise GenConViTHipError(f"frame_hist: regions {regions}; accepted values are 1, 2, 4 and 8")
    if h < regions or w < regions or h * w > 1 << 30:
        raise GenConViTHipError(f"frame_hist: frames of {h}x{w} pixels; each side must be at least regions = {regions} and "
                                f"a frame hold at most 2^30 pixels")
    hist = _out_buffer("frame_hist", out, (nf, regions * regions, CUT_BINS), frames_u8.device)
    check(load().gcv_frame_hist(frames_u8.data_ptr(), nf, h, w, regions, hist.data_ptr(), current_stream_ptr(frames_u8.device)),
          "gcv_frame_hist")
    return hist


def _check_hist(what, hist):
    """``hist`` as a contiguous int32 (F, R^2, 64) device tensor, F >= 1, and (F, R^2, the R its shape implies)."""
    import torch
    squares = [r * r for r in CUT_REGIONS]
    if not (torch.is_tensor(hist) and hist.is_cuda and hist.dtype == torch.int32 and hist.dim() == 3
            and hist.shape[0] >= 1 and hist.shape[2] == CUT_BINS and hist.shape[1] in squares):
        raise GenConViTHipError(f"{what} expects an int32 device tensor of shape (F, R^2, 64), F >= 1, R in 1, 2, 4, 8")
    return hist.contiguous(), int(hist.shape[0]), int(hist.shape[1]), CUT_REGIONS[squares.index(hist.shape[1])]


def hist_diff(hist):
    """L1 distance between the histograms of consecutive frames (``gcv_hist_diff``).  ``hist``: (F, R^2, 64) int32 device
    tensor as ``frame_hist`` returns it, R in 1, 2, 4, 8.  Returns (F - 1, R^2) int32 on the device, empty for F = 1 (nothing
    is launched).  A distance is at most twice the region's pixel count; the one value that does not fit int32, 2^31 (a
    whole frame of 2^30 pixels at R = 1 with disjoint histograms), reads -2^31: view the tensor's numpy array as uint32."""
    import torch
    hist, nf, rr, regions = _check_hist("hist_diff", hist)
    dist = torch.empty((nf - 1, rr), dtype=torch.int32, device=hist.device)
    if nf > 1:
        check(load().gcv_hist_diff(hist.data_ptr(), nf, regions, dist.data_ptr(), current_stream_ptr(hist.device)),
              "gcv_hist_diff")
    return dist


def hist_diff_lag(hist, lag):
    """``hist_diff`` between frames p and p + ``lag`` (``gcv_hist_diff_lag``): (max(F - lag, 0), R^2) int32 on the device,
    nothing launched when it is empty.  ``lag``: an integer >= 1; ``lag`` = 1 is ``hist_diff``."""
    import torch
    hist, nf, rr, regions = _check_hist("hist_diff_lag", hist)
    if isinstance(lag, bool) or not isinstance(lag, int) or lag < 1:
        raise GenConViTHipError(f"hist_diff_lag: lag {lag} must be an integer >= 1")
    dist = torch.empty((max(nf - lag, 0), rr), dtype=torch.int32, device=hist.device)
    if nf > lag:
        check(load().gcv_hist_diff_lag(hist.data_ptr(), nf, regions, lag, dist.data_ptr(), current_stream_ptr(hist.device)),
              "gcv_hist_diff_lag")
    return dist


CELL_GRIDS, CELL_MAX_PIXELS, FIT_LAGS = (8, 16, 32), 1 << 25, (2, 32)


def frame_cells(frames_u8, grid=16, out=None):
    """Luma sums of the ``grid`` x ``grid`` cells of every frame (``gcv_frame_cells``, include/genconvit_hip.h: the arithmetic
    is stated there).  ``frames_u8``: (F,H,W,3) uint8 device tensor (RGB), F >= 1; a slice such as ``frames[1:]`` is used in
    place, whatever its alignment.  Returns (F, grid^2) int32 on the device: the C entry's uint32 sums, which stay below
    2^29.  ``out``: write into this contiguous int32 tensor of that shape on the same device instead of a new one (the rows
    of one group of frames in a whole video's buffer).  ``grid`` other than 8, 16, 32, a frame lower or narrower than
    ``grid``, more than 2^25 pixels a frame (the bound that keeps ``blend_fit``'s 64-bit sums exact), a host tensor and a
    wrong shape or dtype are errors."""
    frames_u8, (nf, h, w) = _check_frames(frames_u8, "frame_cells expects a uint8 device tensor of shape (F,H,W,3), F >= 1", 1)
    if isinstance(grid, bool) or not isinstance(grid, int) or grid not in CELL_GRIDS:
        raise GenConViTHipError(f"frame_cells: grid {grid}; accepted values are 8, 16 and 32")
    if h < grid or w < grid or h * w > CELL_MAX_PIXELS:
        raise GenConViTHipError(f"frame_cells: frames of {h}x{w} pixels; each side must be at least grid = {grid} and a "
                                f"frame hold at most 2^25 pixels")
    cells = _out_buffer("frame_cells", out, (nf, grid * grid), frames_u8.device)
    check(load().gcv_frame_cells(frames_u8.data_ptr(), nf, h, w, grid, cells.data_ptr(), current_stream_ptr(frames_u8.device)),
          "gcv_frame_cells")
    return cells


def blend_fit(cells, lag):
    """How well the frames inside every span of ``lag`` frames lie on the line between the span's ends
    (``gcv_blend_fit``, include/genconvit_hip.h).  ``cells``: (F, G^2) int32 device tensor as ``frame_cells`` returns it, G in
    8, 16, 32, entries non-negative and every row's sum of squares below 2^62 (rows of ``frame_cells`` are); ``lag``: an
    integer in 2 ... 32.  Returns (max(F - lag, 0), 2 lag - 1) int64 on the device, rows [Sdd, Smd_1 ... Smd_(lag-1),
    Smm_1 ... Smm_(lag-1)], exact; nothing is launched when it is empty."""
    import torch
    if not (torch.is_tensor(cells) and cells.is_cuda and cells.dtype == torch.int32 and cells.dim() == 2
            and cells.shape[0] >= 1 and cells.shape[1] in [g * g for g in CELL_GRIDS]):
        raise GenConViTHipError("blend_fit expects an int32 device tensor of shape (F, G^2), F >= 1, G in 8, 16, 32")
    if isinstance(lag, bool) or not isinstance(lag, int) or not FIT_LAGS[0] <= lag <= FIT_LAGS[1]:
        raise GenConViTHipError(f"blend_fit: lag {lag} must be an integer in {FIT_LAGS[0]} ... {FIT_LAGS[1]}")
    cells = cells.contiguous()
    nf, gg = cells.shape
    fit = torch.empty((max(nf - lag, 0), 2 * lag - 1), dtype=torch.int64, device=cells.device)
    if nf > lag:
        check(load().gcv_blend_fit(cells.data_ptr(), nf, CELL_GRIDS[[g * g for g in CELL_GRIDS].index(gg)], lag, fit.data_ptr(),
                                current_stream_ptr(cells.device)), "gcv_blend_fit")
    return fit


_JET = {}


def jet_lut(device=None):
    """The built-in colour map as a (256,3) uint8 tensor: lut[i][c] = rint(255 * clamp(1.5 - |4 i / 255 - (3, 2, 1)[c]|,
    0, 1)), computed in float64 on the host — blue for 0 through green to red for 1.  ``device``: where to put it (kept
    per device, as ``cam_overlay``'s default); None: the host."""
    import torch
    key = None if device is None else str(torch.device(device))
    if key not in _JET:
        i = torch.arange(256, dtype=torch.float64)[:, None]
        c = torch.tensor([3.0, 2.0, 1.0], dtype=torch.float64)[None, :]
        lut = torch.round(255.0 * (1.5 - (4.0 * i / 255.0 - c).abs()).clamp(0.0, 1.0)).to(torch.uint8)
        _JET[key] = lut if device is None else lut.to(device)
    return _JET[key]


def cam_overlay(frames_u8, boxes, maps, alpha=0.5, weighted=True, lut=None, out=None):
    """Draw evidence maps over their face boxes (``gcv_cam_overlay``, include/genconvit_hip.h: the arithmetic is stated
    there).  ``frames_u8``: (F,H,W,3) uint8 device tensor (RGB); ``boxes``: (n,5) integers (frame index, top, right,
    bottom, left), applied in row order; ``maps``: (n,mh,mw) floating point on the same device, one per box, values in
    [0, 1] (``normalize_cams``), 1 <= mh, mw <= 224; ``alpha`` in [0, 1]: the blend weight, scaled by the map value when
    ``weighted``; ``lut``: (256,3) uint8 colours (default ``jet_lut``); ``out``: a contiguous tensor like the frames to
    write into (``out=frames_u8`` draws in place).  Returns the (F,H,W,3) uint8 frames with the overlays drawn."""
    import torch
    src, (nf, h, w) = _check_frames(frames_u8, "cam_overlay: frames must be a uint8 device tensor of shape (F,H,W,3)",
                                    on_device=False)
    dev = frames_u8.device
    b = _check_boxes("cam_overlay", boxes, nf, h, w)
    n = b.shape[0]
    if not (torch.is_tensor(maps) and maps.is_floating_point() and maps.device == dev and maps.dim() == 3):
        raise GenConViTHipError(f"cam_overlay: maps must be a floating-point tensor of shape (n,mh,mw) on {dev}")
    if maps.shape[0] != n:
        raise GenConViTHipError(f"cam_overlay: maps holds {maps.shape[0]} maps for {n} boxes")
    mh, mw = maps.shape[1:]
    if n and not (1 <= mh <= 224 and 1 <= mw <= 224):
        raise GenConViTHipError(f"cam_overlay: maps of {mh}x{mw} cells; 1 ... 224 a side are accepted")
    if not 0.0 <= float(alpha) <= 1.0:
        raise GenConViTHipError(f"cam_overlay: alpha {alpha} outside [0, 1]")
    if lut is None:
        lut = jet_lut(dev)
    elif not (torch.is_tensor(lut) and lut.dtype == torch.uint8 and tuple(lut.shape) == (256, 3) and lut.device == dev):
        raise GenConViTHipError(f"cam_overlay: lut must be a (256,3) uint8 tensor on {dev}")
    if not frames_u8.is_cuda:                # last, so that the checks above do not need a device
        raise GenConViTHipError("cam_overlay: frames must be a uint8 device tensor of shape (F,H,W,3); there is no CPU path")
    if out is None:
        out = torch.empty((nf, h, w, 3), dtype=torch.uint8, device=dev)
    elif not (torch.is_tensor(out) and out.dtype == torch.uint8 and out.shape == frames_u8.shape and out.device == dev
              and out.is_contiguous()):
        raise GenConViTHipError(f"cam_overlay: out must be a contiguous uint8 tensor of shape {tuple(frames_u8.shape)} on {dev}")
    lib = load()
    if nf * h * w == 0:
        return out
    maps, lut, bd = maps.float().contiguous(), lut.contiguous(), b.to(dev)
    check(lib.gcv_cam_overlay(src.data_ptr(), nf, h, w, bd.data_ptr() if n else None, n, maps.data_ptr() if n else None,
                              mh, mw, lut.data_ptr(), float(alpha), 1 if weighted else 0, out.data_ptr(),
                              current_stream_ptr(dev)), "gcv_cam_overlay")
    return out


ANNOTATE_THICK_MAX, ANNOTATE_LABEL_MAX, ANNOTATE_LANES_MAX = 16, 999, 8


def _check_marks(what, marks, nf, h, w):
    """``marks`` as an (n,8) int32 host tensor (``gcv_scan_annotate``, include/genconvit_hip.h); a mark outside its (h, w)
    frame, a ``thick`` outside 1 ... 16, a ``label`` outside -1 ... 999 or a colour outside 0 ... 0xFFFFFF is an error that
    names the row."""
    import torch
    m = torch.as_tensor(marks, dtype=torch.int64).reshape(-1, 8).cpu()
    if m.numel():
        f, top, right, bottom, left, colour, thick, label = m.unbind(1)
        ok = (f >= 0) & (f < nf) & (top >= 0) & (left >= 0) & (bottom <= h) & (right <= w) & (top < bottom) & (left < right)
        for bad, why in ((~ok, f"lies outside its {h}x{w} frame"),
                         ((thick < 1) | (thick > ANNOTATE_THICK_MAX), f"has a thick outside 1 ... {ANNOTATE_THICK_MAX}"),
                         ((label < -1) | (label > ANNOTATE_LABEL_MAX), f"has a label outside -1 ... {ANNOTATE_LABEL_MAX}"),
                         ((colour < 0) | (colour > 0xFFFFFF), "has a colour outside 0 ... 0xFFFFFF")):
            if bool(bad.any()):
                raise GenConViTHipError(f"{what}: mark {int(bad.nonzero()[0])} {why}")
    return m.to(torch.int32)


def scan_annotate(frames_u8, frame_no, marks, timeline=None, strip=0, out=None):
    """Draw a scan's marks and its timeline onto the frames (``gcv_scan_annotate``, include/genconvit_hip.h: the arithmetic
    is stated there).  ``frames_u8``: (F,H,W,3) uint8 device tensor (RGB), of any alignment; ``frame_no``: F integers, each
    frame's number on the timeline; ``marks``: (n,8) integers (frame index, top, right, bottom, left, colour, thick,
    label), applied in row order — colours are packed r | g << 8 | b << 16, ``thick`` is the outline's width and the
    label's cell size in pixels, 1 ... 16, ``label`` a number 0 ... 999 drawn in the box's corner or -1 for none;
    ``timeline``: (L, T) integer tensor of packed colours, 1 <= L <= 8, drawn over the lowest ``strip`` rows of every
    frame, lane l over its share of them, with a white cursor at ``frame_no``; ``strip`` = 0 (then ``timeline`` may be
    None): no timeline; ``out``: a contiguous tensor like the frames to write into (``out=frames_u8`` draws in place).
    Returns the (F,H,W,3) uint8 frames with the drawing."""
    import torch
    src, (nf, h, w) = _check_frames(frames_u8, "scan_annotate: frames must be a uint8 device tensor of shape (F,H,W,3)",
                                    on_device=False)
    dev = frames_u8.device
    m = _check_marks("scan_annotate", marks, nf, h, w)
    n = m.shape[0]
    try:
        fno = torch.as_tensor(frame_no).reshape(-1).cpu()
    except (TypeError, ValueError, RuntimeError):
        fno = None
    if fno is None or fno.is_floating_point() or fno.dtype == torch.bool or fno.numel() != nf:
        raise GenConViTHipError(f"scan_annotate: frame_no must hold {nf} integers, one per frame")
    if isinstance(strip, bool) or not isinstance(strip, int) or strip < 0:
        raise GenConViTHipError(f"scan_annotate: strip {strip} must be an integer >= 0")
    lanes = t = 0
    if strip > 0:
        if not (torch.is_tensor(timeline) and not timeline.is_floating_point() and not timeline.is_complex()
                and timeline.dtype != torch.bool and timeline.dim() == 2 and timeline.shape[0] >= 1 and timeline.shape[1] >= 1):
            raise GenConViTHipError("scan_annotate: timeline must be an (L, T) integer tensor, L, T >= 1")
        lanes, t = (int(v) for v in timeline.shape)
        if lanes > ANNOTATE_LANES_MAX or lanes > strip:
            raise GenConViTHipError(f"scan_annotate: a timeline of {lanes} lanes on a strip of {strip} rows; at most "
                                    f"{ANNOTATE_LANES_MAX} lanes, and no more lanes than rows")
        if strip > h:
            raise GenConViTHipError(f"scan_annotate: a strip of {strip} rows on frames of {h}")
        if t * w >= 1 << 31:
            raise GenConViTHipError(f"scan_annotate: a timeline of T = {t} on frames {w} wide; T * W must stay below 2^31")
    if out is not None and not (torch.is_tensor(out) and out.dtype == torch.uint8 and out.shape == frames_u8.shape
                                and out.device == dev and out.is_contiguous()):
        raise GenConViTHipError(f"scan_annotate: out must be a contiguous uint8 tensor of shape {tuple(frames_u8.shape)} on {dev}")
    if not frames_u8.is_cuda:                # last, so that the checks above do not need a device
        raise GenConViTHipError("scan_annotate: frames must be a uint8 device tensor of shape (F,H,W,3); there is no CPU path")
    if out is None:
        out = torch.empty((nf, h, w, 3), dtype=torch.uint8, device=dev)
    lib = load()
    if nf * h * w == 0:
        return out
    md, fd = m.to(dev), fno.to(torch.int32).to(dev)
    tl = (timeline.to(dev).long() & 0xFFFFFF).to(torch.int32).contiguous() if strip > 0 else None
    check(lib.gcv_scan_annotate(src.data_ptr(), nf, h, w, fd.data_ptr(), md.data_ptr() if n else None, n,
                                tl.data_ptr() if strip > 0 else None, lanes, t, strip, out.data_ptr(),
                                current_stream_ptr(dev)), "gcv_scan_annotate")
    return out


YUV_LAYOUTS, YUV_MATRICES = ("i420", "nv12"), ("bt601", "bt709")      # the C entries' codes are the positions


def _check_yuv_names(what, layout, matrix):
    """The C entries' (layout, matrix) codes; an unknown name is an error."""
    if layout not in YUV_LAYOUTS:
        raise GenConViTHipError(f"{what}: unknown layout {layout!r}; accepted values are 'i420' and 'nv12'")
    if matrix not in YUV_MATRICES:
        raise GenConViTHipError(f"{what}: unknown matrix {matrix!r}; accepted values are 'bt601' and 'bt709'")
    return YUV_LAYOUTS.index(layout), YUV_MATRICES.index(matrix)


def yuv420_geometry(what, shape):
    """(F, H, W) of a (F, 3H/2, W) YUV 4:2:0 buffer; a shape that is none, or an odd H or W, is an error."""
    if len(shape) != 3 or shape[1] < 3 or shape[1] % 3 or shape[2] < 2 or shape[2] % 2:
        raise GenConViTHipError(f"{what}: a shape of {tuple(shape)}; YUV 4:2:0 frames are (F, 3H/2, W) with H and W even and "
                                f"at least 2")
    return int(shape[0]), int(shape[1]) * 2 // 3, int(shape[2])


def yuv420_to_rgb(frames, layout="i420", matrix="bt709", full_range=False, out=None):
    """YUV 4:2:0 frames to RGB (``gcv_yuv420_to_rgb``, include/genconvit_hip.h: the layouts and the arithmetic are stated
    there).  ``frames``: (F, 3H/2, W) uint8 device tensor, one row of 3HW/2 bytes per frame as a decoder delivers it, H and W
    even; a slice such as ``frames[1:]`` is used in place, whatever its alignment.  ``layout``: "i420" or "nv12"; ``matrix``:
    "bt601" or "bt709"; ``full_range``: 0 ... 255 rather than 16 ... 235 / 240.  Returns (F,H,W,3) uint8 RGB on the device;
    ``out``: write into this contiguous uint8 tensor of that shape on the same device instead of a new one.  F = 0 launches
    nothing.  A host tensor, a wrong dtype, rank or shape, odd sizes and unknown names are errors."""
    import torch
    what = "yuv420_to_rgb"
    if not (torch.is_tensor(frames) and frames.dtype == torch.uint8 and frames.dim() == 3):
        raise GenConViTHipError(f"{what} expects a uint8 device tensor of shape (F, 3H/2, W)")
    nf, h, w = yuv420_geometry(what, frames.shape)
    lay, mat = _check_yuv_names(what, layout, matrix)
    if not frames.is_cuda:                   # last, so that the checks above do not need a device
        raise GenConViTHipError(f"{what} expects a uint8 device tensor of shape (F, 3H/2, W); there is no CPU path")
    frames = frames.contiguous()
    rgb = _out_buffer(what, out, (nf, h, w, 3), frames.device, torch.uint8)
    lib = load()
    if nf:
        check(lib.gcv_yuv420_to_rgb(frames.data_ptr(), nf, h, w, lay, mat, 1 if full_range else 0, rgb.data_ptr(),
                                    current_stream_ptr(frames.device)), "gcv_yuv420_to_rgb")
    return rgb


def rgb_to_yuv420(frames, layout="i420", matrix="bt709", full_range=False, out=None):
    """RGB frames to YUV 4:2:0 (``gcv_rgb_to_yuv420``, include/genconvit_hip.h), the reverse of ``yuv420_to_rgb``: ``frames``
    (F,H,W,3) uint8 device tensor, H and W even and at least 2, of any alignment; returns (F, 3H/2, W) uint8 on the device in
    ``layout``, each chroma sample from the sum of its 2 x 2 block.  ``out``: write into this contiguous uint8 tensor of that
    shape on the same device instead of a new one.  F = 0 launches nothing."""
    import torch
    what = "rgb_to_yuv420"
    frames, (nf, h, w) = _check_frames(frames, f"{what} expects a uint8 device tensor of shape (F,H,W,3)", on_device=False)
    if h < 2 or w < 2 or h % 2 or w % 2:
        raise GenConViTHipError(f"{what}: frames of {h}x{w} pixels; H and W must be even and at least 2")
    lay, mat = _check_yuv_names(what, layout, matrix)
    if not frames.is_cuda:                   # last, so that the checks above do not need a device
        raise GenConViTHipError(f"{what} expects a uint8 device tensor of shape (F,H,W,3); there is no CPU path")
    yuv = _out_buffer(what, out, (nf, 3 * h // 2, w), frames.device, torch.uint8)
    lib = load()
    if nf:
        check(lib.gcv_rgb_to_yuv420(frames.data_ptr(), nf, h, w, lay, mat, 1 if full_range else 0, yuv.data_ptr(),
                                    current_stream_ptr(frames.device)), "gcv_rgb_to_yuv420")
    return yuv


def vote_segments(logits, batch, nets, offsets):
    """Per-video ``mean(sigmoid(logits), dim=0)`` for several videos batched in one forward (row N3):
    ``offsets`` = int32 device tensor of n_videos+1 frame offsets; returns (n_videos, 2) fp32."""
    import torch
    lib = load()
    logits = logits.float().contiguous()
    offsets = offsets.to(device=logits.device, dtype=torch.int32).contiguous()
    nvid = offsets.numel() - 1
    out = torch.empty((nvid, 2), dtype=torch.float32, device=logits.device)
    check(lib.gcv_vote_segments(logits.data_ptr(), int(batch), int(nets), offsets.data_ptr(), nvid, out.data_ptr(),
                                current_stream_ptr(logits.device)), "gcv_vote_segments")
    return out


def vote_windows(logits, batch, nets, ranges):
    """Per-frame scores and votes over arbitrary frame ranges (``gcv_vote_windows``).  ``logits``: the (nets * batch, 2)
    rows of one forward, [net 0 frames; net 1 frames]; ``ranges``: (n,2) integers [lo, hi) of frame rows, which may
    overlap, nest, repeat and come in any order (lo < 0, hi > batch or lo > hi is an error).  Returns ``(frame_p, mean2)``:
    (batch,2) fp32 mean over nets of sigmoid per frame, and (n,2) fp32 mean of it over each range (0.5 for an empty one)."""
    import torch
    batch, nets = int(batch), int(nets)
    if not (torch.is_tensor(logits) and logits.is_cuda):
        raise GenConViTHipError("vote_windows expects the logits as a device tensor")
    logits = logits.float().contiguous()
    if nets not in (1, 2) or batch <= 0 or logits.numel() != 2 * nets * batch:
        raise GenConViTHipError(f"vote_windows: {logits.numel()} logits for batch {batch} x {nets} nets x 2")
    r = torch.as_tensor(ranges, dtype=torch.int32).reshape(-1, 2).cpu()
    if r.numel():
        ok = (r[:, 0] >= 0) & (r[:, 1] <= batch) & (r[:, 0] <= r[:, 1])
        if not bool(ok.all()):
            k = int((~ok).nonzero()[0])
            raise GenConViTHipError(f"vote_windows: range {k} [{int(r[k, 0])}, {int(r[k, 1])}) is not inside [0, {batch}]")
    n = r.shape[0]
    frame_p = torch.empty((batch, 2), dtype=torch.float32, device=logits.device)
    mean2 = torch.empty((n, 2), dtype=torch.float32, device=logits.device)
    rd = r.contiguous().to(logits.device)
    check(load().gcv_vote_windows(logits.data_ptr(), batch, nets, rd.data_ptr() if n else None, n, frame_p.data_ptr(),
                                  mean2.data_ptr() if n else None, current_stream_ptr(logits.device)), "gcv_vote_windows")
    return frame_p, mean2


def vote(logits):
    """Device-side ``mean(sigmoid(logits), dim=0)`` (model/pred_func.py:120,125) -> (2,) fp32 tensor."""
    import torch
    lib = load()
    logits = logits.float().contiguous().reshape(-1, 2)
    out = torch.empty((2,), dtype=torch.float32, device=logits.device)
    check(lib.gcv_vote(logits.data_ptr(), logits.shape[0], out.data_ptr(), current_stream_ptr(logits.device)), "gcv_vote")
    return out
