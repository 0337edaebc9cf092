"""ConvNeXt-L timing on one MI355X: genconvit fp16 frames/s at B = 15 and 128 (alternating runs), and the achieved HBM
bandwidth of the two-channels-per-lane depthwise kernel (csrc/dwconv_pair.h) at its four 224-pixel shapes.

    python profiles/large_timing.py [--steps 30] [--rounds 3] [--out profiles/large_timing.json]

Synthetic weights (genconvit_amd.synth), random frames; prints one JSON object and writes it to --out."""
from __future__ import annotations

import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from genconvit_amd import _lib, spec, synth                                  # noqa: E402
from genconvit_amd.model.genconvit import GenConViT                          # noqa: E402
from genconvit_amd.model.genconvit_ed import GenConViTED                      # noqa: E402
from genconvit_amd.model.genconvit_vae import GenConViTVAE                    # noqa: E402
from genconvit_amd.model.config import load_config                           # noqa: E402

HBM_BYTES_PER_S = 8.0e12          # MI355X peak HBM3E bandwidth


def large_model(dtype):
    cfg = load_config()
    cfg["model"]["backbone"] = "convnext_large"
    ed = GenConViTED(cfg, init="empty")
    ed.load_state_dict(synth.make_state_dict(spec.ed_spec("convnext_large"), synth.DEFAULT_SEED, "edL/"))
    vae = GenConViTVAE(cfg, init="empty")
    vae.load_state_dict(synth.make_state_dict(spec.vae_spec(True, "convnext_large"), synth.DEFAULT_SEED, "vaeL/"))
    return GenConViT.from_modules(ed.to("cuda", dtype).eval(), vae.to("cuda", dtype).eval(), "genconvit")


def time_forward(model, B, steps, dtype):
    x = torch.randn((B, 3, 224, 224), device="cuda").to(dtype)
    eps = torch.randn((B, 12544), device="cuda")
    for _ in range(3):
        model(x, eps=eps)
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(steps):
        model(x, eps=eps)
    e1.record()
    torch.cuda.synchronize()
    ms = e0.elapsed_time(e1) / steps
    return ms, B / (ms / 1000.0)


def time_dwconv(C, H, n, dtype, iters=50):
    lib = _lib.load()
    x = torch.randn((n, H, H, C), device="cuda").to(dtype)
    y = torch.empty_like(x)
    w = torch.randn((49, C), device="cuda") * 0.1
    b, lw, lb = torch.zeros(C, device="cuda"), torch.ones(C, device="cuda"), torch.zeros(C, device="cuda")
    s = _lib.current_stream_ptr(torch.device("cuda", 0))
    call = lambda: _lib.check(lib.gcv_k_dwconv7_ln(_lib.dtype_code(dtype), x.data_ptr(), w.data_ptr(), b.data_ptr(),
                                                    lw.data_ptr(), lb.data_ptr(), y.data_ptr(), n, H, H, C, 1e-6, s),
                              "gcv_k_dwconv7_ln")
    for _ in range(5):
        call()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(iters):
        call()
    e1.record()
    torch.cuda.synchronize()
    us = e0.elapsed_time(e1) * 1000.0 / iters
    nbytes = 2.0 * x.numel() * x.element_size()
    return us, nbytes / (us * 1e-6) / HBM_BYTES_PER_S


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=30)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--out", default="profiles/large_timing.json")
    a = ap.parse_args()
    torch.set_grad_enabled(False)
    dtype = torch.float16
    res = {"dwconv_pair": {}, "genconvit_fp16": {"15": [], "128": []}}
    # 256 images: the ED network's two 128-frame passes share one launch
    for C, H in ((192, 56), (384, 28), (768, 14), (1536, 7)):
        us, frac = time_dwconv(C, H, 256, dtype)
        res["dwconv_pair"][f"C{C}_H{H}_n256"] = {"us": round(us, 1), "hbm_fraction": round(frac, 3)}
    model = large_model(dtype)
    for _ in range(a.rounds):                 # alternating batch sizes
        for B in (15, 128):
            ms, fps = time_forward(model, B, a.steps, dtype)
            res["genconvit_fp16"][str(B)].append({"ms": round(ms, 3), "fps": round(fps, 1)})
    print(json.dumps(res))
    os.makedirs(os.path.dirname(a.out) or ".", exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
