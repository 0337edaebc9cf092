"""GenConViTVAE — network B of GenConViT on the MI355X HIP path.

Mirror of the reference's ``model/genconvit_vae.py:91-116``: same class name, constructor arguments,
state_dict keys and ``forward(x) -> (logits (B,2), resized reconstruction (B,3,224,224))`` tuple.
The encoder's only RNG draw (``torch.randn_like``, genconvit_vae.py:46) is an explicit ``eps``
argument here (drawn with ``torch.randn`` when omitted) so results are reproducible and checkable.
"""
from __future__ import annotations

import torch

from .. import spec, synth
from .. import _lib
from ._base import HipModule, backbone_of, build_param_tree


class GenConViTVAE(HipModule):
    def __init__(self, config, pretrained=True, init="synthetic", seed=synth.DEFAULT_SEED):
        super().__init__()
        self.config = config
        self.latent_dims = config["model"]["latent_dims"]
        if self.latent_dims != spec.LATENT_DIMS:
            raise ValueError("latent_dims must be 12544 = 256*7*7 (decoder Unflatten, genconvit_vae.py:81)")
        self.backbone_name = backbone_of(config)
        self._arch = _lib.ARCH_CODES[self.backbone_name]
        build_param_tree(self, spec.vae_spec(include_unused=True, backbone=self.backbone_name), init, seed, "vae/")
        self.num_feature = spec.NUM_BACKBONE_CLASSES * 2
        self.kl = None          # Encoder.kl side effect (genconvit_vae.py:58), filled when want_kl
        self.mse = None
        self._generator = None
        self.keep_kl_weights = True   # False: encoder.var is not packed (inference never reads it, genconvit.py:70,73)

    def set_generator(self, generator):
        """torch.Generator used for eps when none is passed (device generator of the model device)."""
        self._generator = generator

    def _load_into(self, handle):
        handle.load_vae(self.state_dict(), with_var=self.keep_kl_weights)

    @torch.no_grad()
    def forward(self, x, eps=None, want_recon=True, want_mse=False, want_kl=False):
        x = self._prep_input(x)
        B = x.shape[0]
        if B == 0:                                    # empty batch -> empty outputs (no RNG draw, no launch)
            self.kl, self.mse = None, None
            recon = torch.empty((0, 3, 224, 224), dtype=x.dtype, device=x.device) if want_recon else None
            return torch.empty((0, 2), dtype=torch.float32, device=x.device), recon
        if eps is None:
            eps = torch.randn((B, self.latent_dims), dtype=torch.float32, device=x.device, generator=self._generator)
        else:
            eps = eps.to(device=x.device, dtype=torch.float32)
        if B > self._cap:                             # beyond one handle's workspace: consecutive chunks
            chunks = self._chunks(B)
            parts = [self._get_handle(hi - lo).vae_forward(x[lo:hi], eps[lo:hi], want_recon, want_mse, want_kl)
                     for lo, hi in chunks]
            cat = lambda i: torch.cat([p[i] for p in parts]) if parts[0][i] is not None else None
            logits, recon, mse = cat(0), cat(1), cat(2)
            kl = None
            if want_kl:   # Encoder.kl is a mean over the batch (genconvit_vae.py:58): each chunk's mean weighted by its frames
                kl = sum(p[3] * (hi - lo) for p, (lo, hi) in zip(parts, chunks)) / B
        else:
            logits, recon, mse, kl = self._get_handle(B).vae_forward(x, eps, want_recon, want_mse, want_kl)
        self.kl = kl[0] if kl is not None else None
        self.mse = mse
        return logits, recon

    @torch.no_grad()
    def explain(self, x, eps=None, target=None, upsample=True, layer="s3"):
        """Forward + Grad-CAM of the real / fake decision at the last ConvNeXt stage (``gcv_vae_explain``); ``eps`` and
        ``target`` as in ``forward`` / ``GenConViTED.explain``.  Returns ``(logits, cams)``: ``cams['vae']`` (B,7,7) the map
        of backbone(x), ``cams['vae_xhat']`` (B,3,3) that of backbone(x_hat) at 112 px, ``cams['upsampled']`` (B,224,224)
        the first one resized, or None.  ``layer="s2"``: at the output of stage 2 (``gcv_vae_explain_at``), (B,14,14) and
        (B,7,7)."""
        sa, sb = (7, 3) if _lib.explain_layer(layer)[0] == 3 else (14, 7)
        x = self._prep_input(x)
        B = x.shape[0]
        z = lambda *s: torch.empty(s, dtype=torch.float32, device=x.device)
        if B == 0:
            return z(0, 2), {"vae": z(0, sa, sa), "vae_xhat": z(0, sb, sb), "upsampled": z(0, 224, 224) if upsample else None}
        if eps is None:
            eps = torch.randn((B, self.latent_dims), dtype=torch.float32, device=x.device, generator=self._generator)
        else:
            eps = eps.to(device=x.device, dtype=torch.float32)
        parts = [self._get_handle(hi - lo).vae_explain(x[lo:hi], eps[lo:hi], self._target_chunk(target, lo, hi), upsample,
                                                       layer)
                 for lo, hi in self._chunks(B)]
        cat = lambda i: torch.cat([p[i] for p in parts]) if parts[0][i] is not None else None
        cam = cat(1)
        return cat(0), {"vae": cam[:, :sa * sa].reshape(B, sa, sa), "vae_xhat": cam[:, sa * sa:].reshape(B, sb, sb),
                        "upsampled": cat(2)}

    def backbone_forward(self, images):
        images = self._prep_input(images)
        return self._get_handle(images.shape[0]).convnext_forward(1, images)
