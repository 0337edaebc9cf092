"""CPU restatement, in torch, of the arithmetic of gcv_cam_overlay (include/genconvit_hip.h; csrc/overlay.hip), written from
the header's statement: integer sample positions, one fp32 rounding per multiply and add, round-half-even conversions and
an integer blend.  torch's CPU element-wise ops round each result to fp32 and fuse nothing, so the kernel is expected to be
bit-equal to this (tests/test_overlay_gpu.py).  Test infrastructure: the product does not import it."""
import torch


def jet_lut_ref():
    """lut[i][c] = rint(255 * clamp(1.5 - |4 i / 255 - (3, 2, 1)[c]|, 0, 1)) in float64."""
    lut = torch.empty((256, 3), dtype=torch.uint8)
    for i in range(256):
        for c, centre in enumerate((3.0, 2.0, 1.0)):
            lut[i, c] = int(round(255.0 * min(max(1.5 - abs(4.0 * i / 255.0 - centre), 0.0), 1.0)))   # round(): half to even
    return lut


def coef_ref(s, m):
    """Taps and weight along one side: box side ``s`` pixels over ``m`` map cells -> (i0, i1 int64 (s,), l fp32 (s,))."""
    j = torch.arange(s, dtype=torch.int64)
    num = ((2 * j + 1) * m - s).clamp_min(0)
    i0 = num // (2 * s)
    i1 = (i0 + 1).clamp_max(m - 1)
    l = (num - i0 * (2 * s)).to(torch.float32) / torch.tensor(2 * s, dtype=torch.int64).to(torch.float32)
    return i0, i1, l


def sample_ref(map_, h, w):
    """``v`` of the header for every pixel of an (h, w) box: fp32 (h, w) in [0, 1]."""
    M = map_.detach().to("cpu", torch.float32)
    mh, mw = M.shape
    i0, i1, ly = coef_ref(h, mh)
    j0, j1, lx = coef_ref(w, mw)
    lx, ly = lx[None, :], ly[:, None]
    ax, ay = 1.0 - lx, 1.0 - ly
    t0 = M[i0][:, j0] * ax + M[i0][:, j1] * lx
    t1 = M[i1][:, j0] * ax + M[i1][:, j1] * lx
    return (t0 * ay + t1 * ly).clamp(0.0, 1.0)


def blend_ref(region, v, alpha, weighted, lut):
    """The header's k, a8 and integer blend for one box: ``region`` uint8 (h, w, 3), ``v`` fp32 (h, w) -> uint8 (h, w, 3)."""
    k = torch.round(v * 255.0).to(torch.int64)
    a256 = torch.tensor(alpha, dtype=torch.float32) * 256.0
    a = a256 * v if weighted else a256.expand_as(v)
    a8 = torch.round(a).to(torch.int64).clamp(0, 256)[..., None]
    col = lut.to("cpu", torch.int64)[k]
    return ((region.to(torch.int64) * (256 - a8) + col * a8 + 128) >> 8).to(torch.uint8)


def overlay_ref(frames, boxes, maps, alpha=0.5, weighted=True, lut=None):
    """gcv_cam_overlay on the CPU: a copy of ``frames`` (F,H,W,3) uint8 with the boxes drawn in row order, a later box over
    what an earlier one left.  A box outside its frame draws nothing."""
    out = torch.as_tensor(frames).detach().to("cpu").clone()
    nf, H, W, _ = out.shape
    lut = jet_lut_ref() if lut is None else lut.to("cpu")
    for b, (f, top, right, bottom, left) in enumerate(torch.as_tensor(boxes, dtype=torch.int64).reshape(-1, 5).tolist()):
        if not (0 <= f < nf and 0 <= top < bottom <= H and 0 <= left < right <= W):
            continue
        v = sample_ref(maps[b], bottom - top, right - left)
        out[f, top:bottom, left:right] = blend_ref(out[f, top:bottom, left:right], v, alpha, weighted, lut)
    return out
