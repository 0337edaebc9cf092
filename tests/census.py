"""Which launch geometries the networks reach, asked of the library's own planners without a GPU (gcv_dw_plan, gcv_dw_plan2,
gcv_mlp_plan, gcv_convnext_res_ok).  Several kernels take their geometry from the image or token count of the launch: the
rows per band of the depthwise band kernels, the hidden-range split of the C = 384 pw1 kernel and its pw2 tile, the passes per
persistent workgroup of the C = 192 and C = 96 MLP kernels.  reached(arch) walks every depthwise and MLP launch of

  ED                      both passes as one launch: 2 B images at 224
  VAE, merged schedule    B images at 224 and B at 112 in one backbone pass
  VAE, split schedule     the same two segments as two passes
  gcv_convnext_forward    B images at every resolution gcv_convnext_res_ok accepts

at B = 1 ... the handle limit, the way run_convnext (csrc/net_impl.h) lays them out, and returns the geometry keys with the
smallest count that reaches each.  tests/test_host_cpu.py holds them against the case lists of tests/dwcases.py and
tests/kcases.py: a geometry without a kernel-level case fails there, and so does a case that stops reaching its geometry.

Keys
  depthwise band kernels  (kind, C, NS, H, band_rows), per storage dtype.  The tile and whole-map kinds have no geometry that
                          depends on the count beyond the grid's length; tests/dwcases.py covers them per kernel.
  merged launches         (key of group 0, key of group 1); a Tiny<768, 3> group is ("tiny", 768, 3, 3, 0)
  C = 384 pair            (ns, (BN, D, TB) of pw2)
  persistent kernels      (kernel, epilogue, passes): kernel "xs192" or "res96", epilogue "plain" or "lnp", passes the most
                          passes per workgroup (xs192) or tiles per wave (res96) as 1, 2 or 3 (three and more)
"""
import ctypes
import functools

import torch

from genconvit_amd import _lib

DW_KINDS = ("tile", "tiny", "tiny_pair", "roll", "mfma", "pair")      # gcv_dw_plan's kind codes (include/genconvit_hip.h)
BAND_KINDS = ("roll", "mfma", "pair")
MLP_KINDS = ("gemm", "fused96", "xs192", "pair384")                  # gcv_mlp_plan's
DTYPES = {"f32": torch.float32, "f16": torch.float16, "bf16": torch.bfloat16}
ARCHS = {"tiny": (0, (96, 192, 384, 768), 512), "large": (1, (192, 384, 768, 1536), 256)}   # code, widths, handle limit
WG_CAP = 256                                                         # the networks' launches (csrc/mlp_parts.h, kMlpWgCap)


@functools.lru_cache(maxsize=None)
def dw_plan(dt, n, H, W, C):
    """(kind, grid, block, lds, band_rows) of an aligned launch"""
    out = (ctypes.c_int * 5)()
    _lib.check(_lib.load().gcv_dw_plan(_lib.dtype_code(DTYPES[dt]), n, H, W, C, 1, out), "gcv_dw_plan")
    return (DW_KINDS[out[0]],) + tuple(out[1:])


def dw_key(dt, n, H, C):
    """the geometry key of a launch of n square maps, or None for the kinds without one"""
    kind, _, _, _, band_rows = dw_plan(dt, n, H, H, C)
    if kind in BAND_KINDS:
        return (kind, C, H // 7, H, band_rows)
    return ("tiny", C, H, H, 0) if kind == "tiny" else None


@functools.lru_cache(maxsize=None)
def dw_merged(dt, n0, H0, n1, H1, C):
    out = (ctypes.c_int * 1)()
    _lib.check(_lib.load().gcv_dw_plan2(_lib.dtype_code(DTYPES[dt]), n0, H0, H0, n1, H1, H1, C, out), "gcv_dw_plan2")
    return out[0] == 1


@functools.lru_cache(maxsize=None)
def mlp_plan(dt, C, M, wg_cap=WG_CAP):
    """(kind, seven fields by kind) as include/genconvit_hip.h lists them"""
    out = (ctypes.c_int * 8)()
    _lib.check(_lib.load().gcv_mlp_plan(_lib.dtype_code(DTYPES[dt]), C, M, wg_cap, out), "gcv_mlp_plan")
    return (MLP_KINDS[out[0]],) + tuple(out[1:])


def passes_class(n):
    return min(n, 3)


def mlp_keys(dt, C, M, lnp, wg_cap=WG_CAP):
    """the keys of one MLP launch: {("pair384", ns, (BN, D, TB))} or {(kernel, epilogue, passes)} or nothing"""
    p = mlp_plan(dt, C, M, wg_cap)
    if p[0] == "pair384":
        return {("pair384", p[2], (p[4], p[5], p[6]))}
    if p[0] == "xs192":
        return {("xs192", "lnp" if lnp else "plain", passes_class(p[3]))}
    if p[0] == "fused96" and p[1] == 1:
        return {("res96", "lnp" if lnp else "plain", passes_class(p[4]))}
    return set()


def lnp_fuses(dt, C, M, maps):
    """cnx_mlp.h, lnp_plan: the kind has the epilogue at M tokens and every map is even"""
    p = mlp_plan(dt, C, M)
    return all(w % 2 == 0 for w in maps) and (p[0] == "xs192" or (p[0] == "fused96" and p[1] == 1))


def passes(arch, B):
    """the backbone passes of a step at batch B as lists of (images, resolution) segments"""
    code = ARCHS[arch][0]
    lib = _lib.load()
    out = [[(B, 224), (B, 224)], [(B, 224), (B, 112)], [(B, 224)], [(B, 112)]]
    return out + [[(B, res)] for res in range(4, 452, 4) if lib.gcv_convnext_res_ok(code, res) == 1]


def walk(arch, segs, dt):
    """run_convnext's depthwise and MLP launches for one pass: yields ("dw", n, H, C), ("dw2", n0, H0, n1, H1, C) and
    ("mlp", C, M, lnp)"""
    dims = ARCHS[arch][1]
    maps = [res // 4 for _, res in segs]
    for i, C in enumerate(dims):
        groups = []                                       # neighbouring segments of one geometry are one launch
        for (n, _), w in zip(segs, maps):
            if groups and groups[-1][1] == w:
                groups[-1][0] += n
            else:
                groups.append([n, w])
        if len(groups) == 2 and dw_merged(dt, groups[0][0], groups[0][1], groups[1][0], groups[1][1], C):
            yield ("dw2", groups[0][0], groups[0][1], groups[1][0], groups[1][1], C)
        else:
            for n, w in groups:
                yield ("dw", n, w, C)
        M = sum(n * w * w for (n, _), w in zip(segs, maps))
        yield ("mlp", C, M, False)                        # every stage has blocks in front of its last one
        if i < 3 and lnp_fuses(dt, C, M, maps):
            yield ("mlp", C, M, True)
        maps = [w // 2 for w in maps]


@functools.lru_cache(maxsize=None)
def reached(arch):
    """{"dw": {dt: {key: smallest image count}}, "dw2": {dt: {(key0, key1): smallest (n0, n1)}},
    "mlp": {dt: {key: smallest token count}}} over every pass at B = 1 ... the handle limit"""
    out = {"dw": {}, "dw2": {}, "mlp": {}}
    for dt in DTYPES:
        dw, dw2, mlp, seen = {}, {}, {}, set()
        for B in range(1, ARCHS[arch][2] + 1):
            for segs in passes(arch, B):
                for launch in walk(arch, tuple(segs), dt):
                    if launch in seen:
                        continue
                    seen.add(launch)
                    if launch[0] == "dw":
                        _, n, H, C = launch
                        key = dw_key(dt, n, H, C)
                        if key is not None and key[0] in BAND_KINDS:
                            dw[key] = min(dw.get(key, n), n)
                    elif launch[0] == "dw2":
                        _, n0, H0, n1, H1, C = launch
                        key = (dw_key(dt, n0, H0, C), dw_key(dt, n1, H1, C))
                        dw2[key] = min(dw2.get(key, (n0, n1)), (n0, n1))
                        for k, n in zip(key, (n0, n1)):   # each group runs its single launch's bands: that geometry too
                            if k[0] in BAND_KINDS:
                                dw[k] = min(dw.get(k, n), n)
                    elif dt != "f32":
                        _, C, M, lnp = launch
                        for key in mlp_keys(dt, C, M, lnp):
                            mlp[key] = min(mlp.get(key, M), M)
        out["dw"][dt], out["dw2"][dt], out["mlp"][dt] = dw, dw2, mlp
    return out
