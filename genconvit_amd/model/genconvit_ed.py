"""GenConViTED — network A of GenConViT on the MI355X HIP path.

Mirror of the reference's ``model/genconvit_ed.py:64-88`` (same class name, constructor arguments,
state_dict keys and ``forward(images) -> (B,2)`` contract).  The arithmetic — AE encoder/decoder,
two ConvNeXt-T passes over one 2B-image token stream, GELU-MLP head — runs in
``libgenconvit_hip.so`` (``gcv_ed_forward``); nothing here computes on the CPU.
"""
from __future__ import annotations

import torch

from .. import spec, synth
from .. import _lib
from ._base import HipModule, backbone_of, build_param_tree


class GenConViTED(HipModule):
    def __init__(self, config, pretrained=True, init="synthetic", seed=synth.DEFAULT_SEED):
        """``pretrained`` is accepted for signature compatibility: the reference uses it to fetch
        ImageNet weights through timm (genconvit_ed.py:68-69), which needs a network.  Here the
        parameters start from the deterministic synthetic generator (``init='synthetic'``) or
        uninitialised (``init='empty'``, when a checkpoint is loaded right after)."""
        super().__init__()
        self.config = config
        self.backbone_name = backbone_of(config)
        self._arch = _lib.ARCH_CODES[self.backbone_name]
        build_param_tree(self, spec.ed_spec(self.backbone_name), init, seed, "ed/")
        self.num_features = spec.NUM_BACKBONE_CLASSES * 2          # genconvit_ed.py:72

    def _load_into(self, handle):
        handle.load_ed(self.state_dict())

    @torch.no_grad()
    def forward(self, images):
        images = self._prep_input(images)
        if images.shape[0] == 0:                      # an empty batch is an empty result, as with the reference's nn.Modules
            return torch.empty((0, 2), dtype=torch.float32, device=images.device)
        if images.shape[0] > self._cap:
            return torch.cat([self._get_handle(hi - lo).ed_forward(images[lo:hi]) for lo, hi in self._chunks(images.shape[0])])
        return self._get_handle(images.shape[0]).ed_forward(images)

    @torch.no_grad()
    def explain(self, images, eps=None, target=None, upsample=True, layer="s3"):
        """Forward + Grad-CAM of the real / fake decision at the last ConvNeXt stage (``gcv_ed_explain``), or with
        ``layer="s2"`` at the output of stage 2 (``gcv_ed_explain_at``: ``cams['ed']`` is then (B,2,14,14)).  ``target``:
        None (each frame's argmax), a class (0 / 1) or one class per frame.  Returns ``(logits, cams)``: the logits equal
        ``forward``'s; ``cams['ed']`` (B,2,7,7) fp32 maps of the [reconstruction, original] passes (not normalised) and
        ``cams['upsampled']`` (B,224,224) the original pass's map resized like ``F.interpolate(mode='bilinear')``, or None.
        ``eps`` is accepted for a signature shared with the VAE and ignored."""
        side = 7 if _lib.explain_layer(layer)[0] == 3 else 14
        images = self._prep_input(images)
        B = images.shape[0]
        if B > self._cap:
            parts = [self._get_handle(hi - lo).ed_explain(images[lo:hi], self._target_chunk(target, lo, hi), upsample, layer)
                     for lo, hi in self._chunks(B)]
        else:
            parts = [self._get_handle(B).ed_explain(images, target, upsample, layer)] if B else []
        if not parts:
            z = lambda *s: torch.empty(s, dtype=torch.float32, device=images.device)
            return z(0, 2), {"ed": z(0, 2, side, side), "upsampled": z(0, 224, 224) if upsample else None}
        cat = lambda i: torch.cat([p[i] for p in parts]) if parts[0][i] is not None else None
        return cat(0), {"ed": cat(1), "upsampled": cat(2)}

    def backbone_forward(self, images):
        """The ConvNeXt backbone alone (timm ``convnext_tiny`` / ``convnext_large`` forward, call site genconvit_ed.py:82-83)."""
        images = self._prep_input(images)
        return self._get_handle(images.shape[0]).convnext_forward(0, images)
