"""CPU oracle of the Grad-CAM maps (include/genconvit_hip.h, gcv_*_explain), written from the math, not from the kernels.

The backbone ends in global-avg-pool -> LayerNorm2d -> fc, so the gradient of a logit with respect to the stage-3 map
is the same at every position.  ``head_cams`` starts from the stage-3 tokens the oracle stores under the tap name
``<net>.bb.s3.b2`` (oracle/cpu_ref.py), recomputes pool -> LayerNorm -> fc -> activation -> head in fp32 with autograd,
and forms CAM = ReLU(sum_c alpha_c A_c) with alpha = the spatial mean of d logit / d A.  tests/test_cam_cpu.py checks that
shortcut against autograd through the whole oracle forward.
"""
from __future__ import annotations

import torch
import torch.nn.functional as F

# per network: backbone prefix, head activation, stage-3 tokens per image of each pass (cat order), map side
NETS = {
    "ed": ("backbone.", F.gelu, (49, 49)),
    "vae": ("convnext_backbone.", F.relu, (49, 9)),
}
PASSES = {"ed": ("ed.rec", "ed.x"), "vae": ("vae.x", "vae.xhat")}


def _q(w, dtype):
    """A weight as the library stores it: rounded to the 16-bit storage dtype (the fp32 path keeps it)."""
    return w if dtype in (None, torch.float32) else w.to(dtype).float()


def stage3(taps, net, B):
    """The oracle's stage-3 tokens of each pass as (B, hw, 768) fp32."""
    s3 = taps[f"{net}.bb.s3.b2"].detach().float().reshape(-1, 768)
    hw = NETS[net][2]
    return [s3[:B * hw[0]].reshape(B, hw[0], 768), s3[B * hw[0]:].reshape(B, hw[1], 768)]


def _st(x, dtype):
    """x rounded to the storage dtype in value, with the identity as its gradient (the library stores these tensors in
    the storage dtype and evaluates the activation masks at the stored values)."""
    return x if dtype in (None, torch.float32) else x + (x.to(dtype).float() - x).detach()


def head_cams(sd, net, As, target=None, dtype=None, as_stored=False):
    """Grad-CAM of ``target`` (None: argmax, int, or (B,) ints) from the stage-3 maps ``As`` of the two passes.
    ``as_stored``: round the backbone logits and the head input to ``dtype`` where the library stores them.
    Returns (logits (B, 2), [cam of each pass (B, hw)], [alpha of each pass (B, 768)])."""
    prefix, act, _ = NETS[net]
    st = (lambda x: _st(x, dtype)) if as_stored else (lambda x: x)
    As = [A.detach().float().clone().requires_grad_(True) for A in As]
    with torch.enable_grad():
        zs = []
        for A in As:
            y = F.layer_norm(A.mean(1), (768,), sd[prefix + "head.norm.weight"], sd[prefix + "head.norm.bias"], 1e-6)
            zs.append(st(F.linear(st(y), _q(sd[prefix + "head.fc.weight"], dtype), sd[prefix + "head.fc.bias"])))
        f = st(act(torch.cat(zs, 1)))
        h = act(F.linear(f, _q(sd["fc.weight"], dtype), sd["fc.bias"]))
        logits = F.linear(h, sd["fc2.weight"], sd["fc2.bias"])
        t = resolve_target(target, logits)
        grads = torch.autograd.grad(logits.gather(1, t[:, None]).sum(), As)
    alphas = [g.mean(1) for g in grads]
    cams = [F.relu((A.detach() * a[:, None, :]).sum(-1)) for A, a in zip(As, alphas)]
    return logits.detach(), cams, alphas


def backbone_logits(sd, net, As, dtype=None):
    """The backbone logits (B, 2000) in cat order, before the head's activation, from the stage-3 maps."""
    prefix = NETS[net][0]
    zs = [F.linear(F.layer_norm(A.float().mean(1), (768,), sd[prefix + "head.norm.weight"], sd[prefix + "head.norm.bias"],
                                1e-6), _q(sd[prefix + "head.fc.weight"], dtype), sd[prefix + "head.fc.bias"]) for A in As]
    return torch.cat(zs, 1)


def resolve_target(target, logits):
    B = logits.shape[0]
    if target is None:
        return logits.argmax(1)
    t = torch.as_tensor(target, dtype=torch.long).reshape(-1)
    return (t.expand(B) if t.numel() == 1 else t).ne(0).long()


def upsample(cam, side):
    """The library's cam224 of a (B, side*side) map: F.interpolate(bilinear, align_corners=False) to 224 x 224."""
    return F.interpolate(cam.reshape(-1, 1, side, side), size=(224, 224), mode="bilinear", align_corners=False)[:, 0]


def map_error(got, want):
    """max |got - want| / rms(want) over the maps of one pass (an all-zero ReLU map has no rms of its own)."""
    rms = want.float().pow(2).mean().sqrt().clamp_min(1e-30)
    return ((got.float() - want.float()).abs().max() / rms).item()
