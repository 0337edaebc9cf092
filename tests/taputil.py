"""Stage-by-stage checks of the networks: the library's taps (include/genconvit_hip.h, gcv_tap_set) against the oracle's
(oracle/cpu_ref.py, ``taps=``), element by element, in the same layout.

The error of a tap is max |got - want| over its elements divided by the RMS of ``want`` (the oracle), so one bound per
tap kind holds across the stages whose activations grow.  A failing tap names its worst element as
(tap, segment, image, token, channel).
"""
from __future__ import annotations

import math

import torch

CONVNEXT_DEPTHS = (3, 3, 9, 3)
CONVNEXT_DIMS = (96, 192, 384, 768)
# backbone segments in the library's concatenation order: (label, resolution)
BB_SEGMENTS = {"ed": (("rec", 224), ("x", 224)), "vae": (("x", 224), ("xhat", 112))}
# network-level taps: name -> (tokens per image, channels, fp32?)
NET_TAPS = {
    "ed": {"ed.e1": (112 * 112, 16, False), "ed.e2": (56 * 56, 32, False), "ed.e3": (28 * 28, 64, False),
           "ed.e4": (14 * 14, 128, False), "ed.e5": (7 * 7, 256, False), "ed.d1": (14 * 14, 128, False),
           "ed.d2": (28 * 28, 64, False), "ed.d3": (56 * 56, 32, False), "ed.d4": (112 * 112, 16, False),
           "ed.rec": (224 * 224, 3, False), "ed.feat": (1, 2000, False)},
    "vae": {"vae.v1": (112 * 112, 16, False), "vae.v2": (56 * 56, 32, False), "vae.v3": (28 * 28, 64, False),
            "vae.v4": (14 * 14, 128, False), "vae.mu": (1, 12544, True), "vae.z": (7 * 7, 256, False),
            "vae.d1": (14 * 14, 64, False), "vae.d2": (28 * 28, 32, False), "vae.d3": (56 * 56, 16, False),
            "vae.xhat": (112 * 112, 3, False), "vae.feat": (1, 2000, False)},
}


# BOUNDS[dtype][group(name)]: about 3x the largest err/rms measured on the MI355X over the configurations of
# tests/test_taps_gpu.py (the measured value in the comment; fp32: ED B = 32 only, with a floor of 1e-5 for the host's
# float32 reductions, whose order depends on its vector ISA and thread count).  The 16-bit errors are one storage-dtype
# rounding of the largest elements apart (bf16: 8 mantissa bits, so |x| / 128 at |x| ~ 12 rms).
BOUNDS = {
    torch.float32: {
        "ed.d1": 1.8e-05,               # 5.70e-06
        "ed.d2": 1.7e-05,               # 5.50e-06
        "ed.d3": 2e-05,                 # 6.47e-06
        "ed.d4": 2.8e-05,               # 9.09e-06
        "ed.e1": 1e-05,                 # 0.00e+00
        "ed.e2": 1e-05,                 # 1.74e-06
        "ed.e3": 1.6e-05,               # 5.26e-06
        "ed.e4": 1.8e-05,               # 5.82e-06
        "ed.e5": 1.8e-05,               # 5.86e-06
        "ed.feat": 2.5e-05,             # 8.24e-06
        "ed.rec": 3e-05,                # 9.95e-06
        "bb.pool": 1e-05,               # 2.49e-06
        "bb.s0.b": 3e-05,               # 9.67e-06
        "bb.s1.b": 1.9e-05,             # 6.11e-06
        "bb.s1.down_in": 3.4e-05,       # 1.13e-05
        "bb.s2.b": 2.6e-05,             # 8.54e-06
        "bb.s2.down_in": 2.8e-05,       # 9.13e-06
        "bb.s3.b": 2.8e-05,             # 9.20e-06
        "bb.s3.down_in": 2.7e-05,       # 8.85e-06
        "bb.stem": 3e-05,               # 9.91e-06
    },
    torch.float16: {
        "ed.d1": 0.019,                 # 6.23e-03
        "ed.d2": 0.02,                  # 6.44e-03
        "ed.d3": 0.019,                 # 6.04e-03
        "ed.d4": 0.026,                 # 8.40e-03
        "ed.e1": 0.0074,                # 2.46e-03
        "ed.e2": 0.0072,                # 2.38e-03
        "ed.e3": 0.0087,                # 2.88e-03
        "ed.e4": 0.012,                 # 3.67e-03
        "ed.e5": 0.014,                 # 4.36e-03
        "ed.feat": 0.017,               # 5.52e-03
        "ed.rec": 0.038,                # 1.27e-02
        "vae.d1": 0.015,                # 4.72e-03
        "vae.d2": 0.022,                # 7.16e-03
        "vae.d3": 0.028,                # 9.09e-03
        "vae.feat": 0.017,              # 5.51e-03
        "vae.mu": 0.0091,               # 3.01e-03
        "vae.v1": 0.026,                # 8.61e-03
        "vae.v2": 0.016,                # 5.00e-03
        "vae.v3": 0.017,                # 5.42e-03
        "vae.v4": 0.025,                # 8.09e-03
        "vae.xhat": 0.02,               # 6.34e-03
        "vae.z": 0.011,                 # 3.35e-03
        "bb.pool": 0.012,               # 3.76e-03
        "bb.s0.b": 0.043,               # 1.41e-02
        "bb.s1.b": 0.028,               # 9.01e-03
        "bb.s1.down_in": 0.048,         # 1.59e-02
        "bb.s2.b": 0.041,               # 1.34e-02
        "bb.s2.down_in": 0.035,         # 1.14e-02
        "bb.s3.b": 0.033,               # 1.09e-02
        "bb.s3.down_in": 0.057,         # 1.88e-02
        "bb.stem": 0.042,               # 1.40e-02
    },
    torch.bfloat16: {
        "ed.d1": 0.15,                  # 4.99e-02
        "ed.d2": 0.12,                  # 3.86e-02
        "ed.d3": 0.15,                  # 4.68e-02
        "ed.d4": 0.21,                  # 6.72e-02
        "ed.e1": 0.06,                  # 1.97e-02
        "ed.e2": 0.057,                 # 1.90e-02
        "ed.e3": 0.07,                  # 2.30e-02
        "ed.e4": 0.089,                 # 2.93e-02
        "ed.e5": 0.11,                  # 3.49e-02
        "ed.feat": 0.1,                 # 3.31e-02
        "ed.rec": 0.27,                 # 8.87e-02
        "vae.d1": 0.12,                 # 3.77e-02
        "vae.d2": 0.18,                 # 5.76e-02
        "vae.d3": 0.17,                 # 5.46e-02
        "vae.feat": 0.14,               # 4.40e-02
        "vae.mu": 0.068,                # 2.25e-02
        "vae.v1": 0.21,                 # 6.89e-02
        "vae.v2": 0.13,                 # 4.01e-02
        "vae.v3": 0.14,                 # 4.34e-02
        "vae.v4": 0.2,                  # 6.47e-02
        "vae.xhat": 0.16,               # 5.07e-02
        "vae.z": 0.17,                  # 5.36e-02
        "bb.pool": 0.091,               # 3.01e-02
        "bb.s0.b": 0.3,                 # 9.95e-02
        "bb.s1.b": 0.19,                # 6.29e-02
        "bb.s1.down_in": 0.27,          # 8.90e-02
        "bb.s2.b": 0.28,                # 9.19e-02
        "bb.s2.down_in": 0.27,          # 8.82e-02
        "bb.s3.b": 0.27,                # 8.67e-02
        "bb.s3.down_in": 0.37,          # 1.21e-01
        "bb.stem": 0.31,                # 1.01e-01
    },
}


def layout(net, B):
    """name -> (fp32?, [(segment label, images, tokens per image, channels), ...]) for every tap of ``net`` at batch B, in
    data-flow order (so the first failing tap is where an error enters)."""
    out = {n: (f32, [("-", B, t, c)]) for n, (t, c, f32) in NET_TAPS[net].items() if not n.endswith(".feat")}
    segs = BB_SEGMENTS[net]

    def bb(what, tokens_at, ch):
        out[f"{net}.bb.{what}"] = (False, [(lab, B, tokens_at(res), ch) for lab, res in segs])

    hw = lambda i: (lambda res: ((res // 4) >> i) ** 2)
    bb("stem", hw(0), 96)
    for i, depth in enumerate(CONVNEXT_DEPTHS):
        if i > 0:
            bb(f"s{i}.down_in", hw(i), 4 * CONVNEXT_DIMS[i - 1])
        for j in range(depth):
            bb(f"s{i}.b{j}", hw(i), CONVNEXT_DIMS[i])
    bb("pool", lambda res: 1, 768)
    out[f"{net}.feat"] = (False, [("-", B, 1, 2000)])
    return out


def group(name):
    """Bound key of a tap: backbone taps of both networks share one key per stage and kind (blocks of a stage together)."""
    if ".bb." not in name:
        return name
    what = name.split(".bb.")[1]
    if ".b" in what:
        what = what.split(".b")[0] + ".b"
    return "bb." + what


def set_taps(handle, net, B, dtype):
    """Register a device buffer for every tap of ``net`` on ``handle``; returns name -> buffer (flat)."""
    bufs = {}
    for name, (f32, segs) in layout(net, B).items():
        n = sum(s[1] * s[2] * s[3] for s in segs)
        bufs[name] = torch.full((n,), float("nan"), dtype=torch.float32 if f32 else dtype, device="cuda")
        handle.set_tap(name, bufs[name])
    return bufs


def locate(segs, flat_index):
    """(segment label, image, token, channel) of element ``flat_index`` of a tap."""
    i = int(flat_index)
    for lab, n, t, c in segs:
        if i < n * t * c:
            return lab, i // (t * c), (i // c) % t, i % c
        i -= n * t * c
    raise IndexError(flat_index)


def compare(got, want, lay, bounds, written=None):
    """One row per tap of ``lay``: dict(name, err, bound, ok, where, ...).

    got: name -> flat tensor (any dtype/device) or None; want: the oracle's taps (None = never stored); written:
    name -> the library's written flag (checked against the oracle's view of the dispatch when given)."""
    rows = []
    for name, (_, segs) in lay.items():
        w = want[name]
        row = {"name": name, "group": group(name), "bound": bounds.get(group(name))}
        if written is not None and written[name] != (w is not None):
            row.update(ok=False, err=math.inf, where=f"library written={written[name]}, oracle stored={w is not None}")
            rows.append(row)
            continue
        if w is None:
            row.update(ok=True, err=None, where="not stored by this dispatch")
            rows.append(row)
            continue
        g = got[name].detach().float().cpu().reshape(-1)
        w = w.detach().float().reshape(-1)
        assert g.numel() == w.numel(), (name, g.numel(), w.numel())
        d = (g - w).abs()
        d[torch.isnan(d)] = math.inf
        k = int(torch.argmax(d))
        rms = float(w.square().mean().sqrt())
        err = float(d[k]) / max(rms, 1e-30)
        lab, img, tok, ch = locate(segs, k)
        row.update(err=err, rms=rms, got=float(g[k]), want=float(w[k]), seg=lab, img=img, tok=tok, ch=ch,
                   where=f"{name} segment {lab} image {img} token {tok} channel {ch}: got {float(g[k]):.6g}, "
                         f"want {float(w[k]):.6g}, |diff|/rms {err:.3e}")
        row["ok"] = row["bound"] is not None and err <= row["bound"]
        rows.append(row)
    return rows


def failures(rows):
    return [r for r in rows if not r["ok"]]


def report(rows, title):
    lines = [title]
    for r in rows:
        e = "-" if r["err"] is None else f"{r['err']:.3e}"
        b = "-" if r["bound"] is None else f"{r['bound']:.1e}"
        lines.append(f"  {r['name']:<22} err/rms {e:>10}  bound {b:>8}  {'ok' if r['ok'] else 'FAIL ' + r['where']}")
    return "\n".join(lines)
