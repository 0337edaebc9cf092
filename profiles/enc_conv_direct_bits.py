#!/usr/bin/env python3
"""Bit-identity of the direct 3x3 convolution kernel (csrc/conv_direct.h) against the parent commit's gemm_kernel path.

    enc_conv_direct_bits.py <parent library> <new library> [--bench]

One fresh process per library (GCV_LIB_PATH) runs the four encoder layers at the network's own shapes (128 frames) on the
same seeded random inputs, fp16 and bf16, through gcv_k_gemm and saves the raw 16-bit outputs; this process compares them with
np.array_equal.  --bench does the same for the logits and the vote of `bench.py --dump-outputs` (fp16, 128 frames).
A mismatch means the accumulation order differs, not that a tolerance is too tight.  Result: enc_conv_direct_bits.txt."""
import os
import shutil
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LAYERS = [("ed 16->32 pool 112", "pool", 112, 16, 32), ("ed 32->64 pool 56", "pool", 56, 32, 64),
          ("vae 16->32 s2 112", "s2", 112, 16, 32), ("vae 32->64 s2 56", "s2", 56, 32, 64)]
FRAMES = 128


def dump(outdir):
    import math
    import numpy as np
    import torch
    sys.path.insert(0, ROOT)
    from genconvit_amd import _lib
    from tests.kutil import dev, gemm, rnd
    for dt, dtype in (("f16", torch.float16), ("bf16", torch.bfloat16)):
        for i, (name, mode, H, cin, cout) in enumerate(LAYERS):
            x = rnd((FRAMES, H, H, cin), 10 + i).to(dev(), dtype)
            w = rnd((cout, 9 * cin), 20 + i, 1 / math.sqrt(9 * cin)).to(dev(), dtype)
            b = rnd((cout,), 30 + i, 0.2).to(dev())
            Ho = H // 2
            out = torch.zeros((FRAMES, Ho, Ho, cout), dtype=dtype, device=dev())
            if mode == "pool":
                gemm(dtype, _lib.A_IM2COL3_POOL, _lib.EPI_POOL4, x, w, out, FRAMES * H * H, cout, 9 * cin, ldc=cout, bias=b,
                     act=1, H=H, W=H, cin_log2=int(math.log2(cin)))
            else:
                gemm(dtype, _lib.A_IM2COL3_S2, _lib.EPI_BIAS_ACT, x, w, out, FRAMES * Ho * Ho, cout, 9 * cin, ldc=cout, bias=b,
                     act=3, H=H, W=H, cin_log2=int(math.log2(cin)))
            np.save(os.path.join(outdir, f"{dt}_{i}.npy"), out.view(torch.int16).cpu().numpy())


def main():
    import numpy as np
    parent, new = os.path.abspath(sys.argv[1]), os.path.abspath(sys.argv[2])
    tmp = tempfile.mkdtemp(prefix="conv_direct_bits_")
    ok = True
    try:
        for tag, lib in (("parent", parent), ("new", new)):
            d = os.path.join(tmp, tag)
            os.makedirs(d)
            env = dict(os.environ, GCV_LIB_PATH=lib)
            subprocess.run([sys.executable, os.path.abspath(__file__), "--dump", d], check=True, env=env, cwd=ROOT, timeout=300)
            if "--bench" in sys.argv:
                subprocess.run([sys.executable, "bench.py", "--gpus", "1", "--steps", "2", "--warmup", "1", "--no-cpu-baseline",
                                "--dump-outputs", os.path.join(d, "bench")], check=True, env=env, cwd=ROOT, timeout=600,
                               stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL)
        for dt in ("f16", "bf16"):
            for i, (name, *_rest) in enumerate(LAYERS):
                a, b = (np.load(os.path.join(tmp, t, f"{dt}_{i}.npy")) for t in ("parent", "new"))
                same = np.array_equal(a, b)
                ok &= same
                print(f"{dt:4s} {name:20s} {a.size:9d} values, {int((a != 0).sum()):9d} non-zero  array_equal: {same}"
                      + ("" if same else f"  ({int((a != b).sum())} differ)"))
        if "--bench" in sys.argv:
            for f in ("logits", "vote"):
                a, b = (np.load(os.path.join(tmp, t, "bench", f"{f}.npy")) for t in ("parent", "new"))
                same = np.array_equal(a, b)
                ok &= same
                print(f"bench.py fp16 {f:7s} {a.shape}  array_equal: {same}")
    finally:
        shutil.rmtree(tmp, ignore_errors=True)
    print("ALL IDENTICAL" if ok else "MISMATCH")
    sys.exit(0 if ok else 1)


if __name__ == "__main__":
    if len(sys.argv) == 3 and sys.argv[1] == "--dump":
        dump(sys.argv[2])
    else:
        main()
