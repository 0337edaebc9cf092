"""CPU oracle of the Grad-CAM maps at the output of ConvNeXt stage 2 (include/genconvit_hip.h, gcv_*_explain_at with
layer = 2), written from the math and from oracle/cpu_ref.py's primitives, not from the kernels.

``s2_cams`` starts from the stage-2 output of each pass (tap ``<net>.bb.s2.b8``; ``...s2.b26`` on ConvNeXt-L), runs the
stage 2 -> 3 down-sampling (LayerNorm2d, 2 x 2 stride-2 conv), stage 3's three blocks, global average pool, LayerNorm, fc,
the activation and the head with autograd, and forms

    alpha_c   = mean over (h, w) of d logit_target / d A2_c(h, w)
    CAM(h, w) = ReLU(sum_c alpha_c A2_c(h, w))

Storage rounding enters as in ``camutil._st``: where the library stores a tensor in its 16-bit dtype the value is rounded
and the gradient is the identity, and derivatives (GELU', the LayerNorm statistics) are taken at the stored values.  The
hidden pre-activation of a block is such a point in the explain path (it is recomputed and stored), while the forward
applies GELU to the unrounded sum: ``_gelu_at`` keeps both.  tests/test_cam2_cpu.py checks the whole against autograd
through the complete oracle forward.
"""
from __future__ import annotations

import torch
import torch.nn.functional as F

from oracle import cpu_ref
from tests import camutil
from tests.camutil import _q, _st

# per architecture: (C2, C3, index of the last stage-2 block)
ARCHS = {"tiny": (384, 768, 8), "large": (768, 1536, 26)}
# stage-2 map side of each pass (cat order)
SIDES = {"ed": (14, 14), "vae": (14, 7)}


def s2_name(net, arch="tiny"):
    return f"{net}.bb.s2.b{ARCHS[arch][2]}"


def split_rows(rows, B, sides, C):
    """Token rows (sum_p B * side_p^2, C) of the passes of one network, in the library's concatenation order, as
    [(B, C, side, side) fp32 per pass]."""
    rows = rows.detach().float().reshape(-1, C)
    out, o = [], 0
    for s in sides:
        n = B * s * s
        out.append(rows[o:o + n].reshape(B, s, s, C).permute(0, 3, 1, 2).contiguous())
        o += n
    assert o == rows.shape[0], (o, rows.shape)
    return out


def stage2(taps, net, B, arch="tiny"):
    """The stage-2 output of each pass as (B, C2, side, side) fp32, from a dict of taps in the library's layout."""
    return split_rows(taps[s2_name(net, arch)], B, SIDES[net], ARCHS[arch][0])


def stage3_blocks(taps, net, B, arch="tiny"):
    """[[block j's output of each pass as (B, C3, side / 2, side / 2)] for j = 0, 1, 2] from taps ``<net>.bb.s3.b<j>``."""
    sides = tuple(s // 2 for s in SIDES[net])
    return [split_rows(taps[f"{net}.bb.s3.b{j}"], B, sides, ARCHS[arch][1]) for j in range(3)]


def _sub(x, value):
    """``value`` with the gradient of ``x``: the library's own stored tensor in the place of the oracle's."""
    return x if value is None else x + (value - x).detach()


def _gelu_at(pre, dtype):
    """GELU(pre) in value, with its derivative taken at ``pre`` as stored (rounded to ``dtype``)."""
    r = _st(pre, dtype)
    return F.gelu(r) + (F.gelu(pre) - F.gelu(r)).detach()


def _block(sd, p, x, dtype, st):
    """cpu_ref.convnext_block with autograd and the explain path's storage points (NCHW in, NCHW out)."""
    c = x.shape[1]
    y = F.conv2d(x, sd[p + "conv_dw.weight"], sd[p + "conv_dw.bias"], padding=3, groups=c).permute(0, 2, 3, 1)
    y = st(F.layer_norm(y, (c,), sd[p + "norm.weight"], sd[p + "norm.bias"], cpu_ref.LN_EPS_CONVNEXT))
    pre = F.linear(y, _q(sd[p + "mlp.fc1.weight"], dtype), sd[p + "mlp.fc1.bias"])
    h = st(_gelu_at(pre, dtype) if st is not _ident else F.gelu(pre))
    y = F.linear(h, _q(sd[p + "mlp.fc2.weight"], dtype), sd[p + "mlp.fc2.bias"]).permute(0, 3, 1, 2)
    return st(y * sd[p + "gamma"].reshape(1, -1, 1, 1) + x)


def _ident(x):
    return x


def s2_cams(sd, net, A2s, target=None, dtype=None, as_stored=False, lib_blocks=None):
    """Grad-CAM of ``target`` (None: argmax, int, or (B,) ints) at the stage-2 maps ``A2s`` ((B, C2, h, w) per pass).
    ``as_stored``: round the activations to ``dtype`` where the library stores them.  ``lib_blocks``: the library's own
    outputs of stage 3's blocks (``stage3_blocks``), substituted in value for the oracle's.
    Returns a dict: logits (B, 2); cams [(B, h * w) per pass]; alphas [(B, C2)]; and the same at the stage-3 output,
    cams3 / alphas3, for the comparison with camutil.head_cams."""
    prefix, act, _ = camutil.NETS[net]
    st = (lambda x: _st(x, dtype)) if as_stored and dtype not in (None, torch.float32) else _ident
    A2s = [A.detach().float().clone().requires_grad_(True) for A in A2s]
    with torch.enable_grad():
        zs, A3s = [], []
        for pi, A in enumerate(A2s):
            x = st(cpu_ref._ln2d(A, sd[prefix + "stages.3.downsample.0.weight"], sd[prefix + "stages.3.downsample.0.bias"],
                                 cpu_ref.LN_EPS_CONVNEXT))
            x = st(F.conv2d(x, _q(sd[prefix + "stages.3.downsample.1.weight"], dtype),
                            sd[prefix + "stages.3.downsample.1.bias"], stride=2))
            for j in range(3):
                x = _block(sd, prefix + f"stages.3.blocks.{j}.", x, dtype, st)
                x = _sub(x, None if lib_blocks is None else lib_blocks[j][pi])
            A3s.append(x)
            C3 = x.shape[1]
            y = F.layer_norm(x.mean((2, 3)), (C3,), sd[prefix + "head.norm.weight"], sd[prefix + "head.norm.bias"],
                             cpu_ref.LN_EPS_CONVNEXT)
            zs.append(st(F.linear(st(y), _q(sd[prefix + "head.fc.weight"], dtype), sd[prefix + "head.fc.bias"])))
        f = st(act(torch.cat(zs, 1)))
        h = act(F.linear(f, _q(sd["fc.weight"], dtype), sd["fc.bias"]))
        logits = F.linear(h, sd["fc2.weight"], sd["fc2.bias"])
        t = camutil.resolve_target(target, logits)
        grads = torch.autograd.grad(logits.gather(1, t[:, None]).sum(), A2s + A3s)
    n = len(A2s)
    out = {"logits": logits.detach()}
    for key, As, gs in (("", A2s, grads[:n]), ("3", A3s, grads[n:])):
        alphas = [g.mean((2, 3)) for g in gs]
        out["alphas" + key] = alphas
        out["cams" + key] = [F.relu((A.detach() * a[:, :, None, None]).sum(1)).flatten(1) for A, a in zip(As, alphas)]
        out["grads" + key] = list(gs)
    return out


def upsample(cam, side):
    return camutil.upsample(cam, side)
