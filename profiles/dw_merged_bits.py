#!/usr/bin/env python3
"""Bit-identity of the network outputs with the two-group depthwise launch (csrc/dwconv_impl.h, launch_dwconv7_ln2)
against the parent commit.

    dw_merged_bits.py <parent tree> <new tree>

Each tree is a checkout with its library built.  One fresh process per tree and configuration runs that tree's
`bench.py --dump-outputs` with GCV_LIB_PATH pointing at that tree's library, and this process compares the logits and the
vote of the last timed step with np.array_equal.  (Whole trees, not two libraries under one genconvit_amd/_lib.py: the new
_lib.py binds gcv_k_dwconv7_ln2, which the parent's library does not export.)

Configurations: the flagship (genconvit, 128 frames) in fp16 and bf16, two streams and --no-concurrent; --net vae
--batch 32 --dtype bf16 as bench.py runs it (the two backbone passes on two streams: one geometry group each, the merged
launch is not reached) and with GCV_VAE_SPLIT=0 (one stream, both segments in one pass: the merged launch at batch 32).
A mismatch means different arithmetic, not a tolerance that is too tight.  Result: dw_merged_bits.txt."""
import os
import shutil
import subprocess
import sys
import tempfile

CONFIGS = [
    ("genconvit b128 f16", ["--dtype", "f16"], {}),
    ("genconvit b128 f16 serial", ["--dtype", "f16", "--no-concurrent"], {}),
    ("genconvit b128 bf16", ["--dtype", "bf16"], {}),
    ("genconvit b128 bf16 serial", ["--dtype", "bf16", "--no-concurrent"], {}),
    ("vae b32 bf16", ["--net", "vae", "--batch", "32", "--dtype", "bf16"], {}),
    ("vae b32 bf16 one stream", ["--net", "vae", "--batch", "32", "--dtype", "bf16"], {"GCV_VAE_SPLIT": "0"}),
]


def main():
    import numpy as np
    trees = {"parent": os.path.abspath(sys.argv[1]), "new": os.path.abspath(sys.argv[2])}
    tmp = tempfile.mkdtemp(prefix="dw_merged_bits_")
    ok = True
    try:
        for i, (name, args, extra) in enumerate(CONFIGS):
            for tag, tree in trees.items():
                lib = os.path.join(tree, "genconvit_amd", "lib", "libgenconvit_hip.so")
                env = dict(os.environ, GCV_LIB_PATH=lib, **extra)
                subprocess.run([sys.executable, "bench.py", "--gpus", "1", "--steps", "2", "--warmup", "1", "--no-cpu-baseline",
                                "--dump-outputs", os.path.join(tmp, tag, str(i))] + args, check=True, env=env, cwd=tree,
                               timeout=300, stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL)
            for f in ("logits", "vote"):
                a, b = (np.load(os.path.join(tmp, t, str(i), f"{f}.npy")) for t in trees)
                same = np.array_equal(a, b) and bool(np.isfinite(a).all())
                ok &= same
                print(f"{name:28s} {f:7s} {str(a.shape):12s} array_equal: {same}", flush=True)
    finally:
        shutil.rmtree(tmp, ignore_errors=True)
    print("ALL IDENTICAL" if ok else "MISMATCH")
    sys.exit(0 if ok else 1)


if __name__ == "__main__":
    main()
