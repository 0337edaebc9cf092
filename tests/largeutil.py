"""ConvNeXt-L (timm 0.6.5 ``convnext_large``) restatement for the tests, built from the oracle's primitives.

``oracle.cpu_ref.convnext_tiny`` is width-generic but takes Tiny's depths and Tiny's 16-bit storage points.  The Large
path of the library (csrc/net_impl.h with a GCV_CONVNEXT_LARGE handle) stores its activations at these points:
* stage 0 (C = 192) runs the Xs192 MLP, whose epilogue applies stage 1's LayerNorm2d + patchify when the maps are even, so
  the last stage-0 block's output is not stored then;
* stage 1 (C = 384) runs the Pair384 MLP, which folds gamma into the packed fc2 (``cpu_ref.convnext_block`` keys that on
  C = 384 already) and has no LayerNorm-patchify epilogue;
* stages 2 and 3 run the tile GEMMs; no depthwise taps are an MFMA operand.
The fp32 path stores everything and rounds nothing, like the oracle.  ``use_large(monkeypatch)`` substitutes it for
``cpu_ref.convnext_tiny`` so that ``cpu_ref.ed_forward`` / ``vae_forward`` describe the Large networks.
"""
from __future__ import annotations

import torch
import torch.nn.functional as F

from genconvit_amd import spec, synth
from oracle import cpu_ref

LARGE_DEPTHS = spec.CONVNEXT_LARGE_DEPTHS
LARGE_DIMS = spec.CONVNEXT_LARGE_DIMS


def convnext_large(sd, prefix, x, taps=None, store_out=True, launch=None, seg_taps=None):
    """timm 0.6.5 ``convnext_large`` forward with the Large path's storage points (signature of cpu_ref.convnext_tiny)."""
    q, p = cpu_ref._q, prefix
    x = F.conv2d(x, sd[p + "stem.0.weight"], sd[p + "stem.0.bias"], stride=4)
    x = q(cpu_ref._ln2d(x, sd[p + "stem.1.weight"], sd[p + "stem.1.bias"], cpu_ref.LN_EPS_CONVNEXT))
    if taps is not None:
        taps["stem"] = x
    if seg_taps is not None:
        seg_taps["stem"] = cpu_ref._rows(x)
    for i, depth in enumerate(LARGE_DEPTHS):
        if i > 0:
            x = q(cpu_ref._ln2d(x, sd[p + f"stages.{i}.downsample.0.weight"], sd[p + f"stages.{i}.downsample.0.bias"],
                                cpu_ref.LN_EPS_CONVNEXT))
            if seg_taps is not None:
                seg_taps[f"s{i}.down_in"] = cpu_ref._patch_rows(x)
            x = q(F.conv2d(x, q(sd[p + f"stages.{i}.downsample.1.weight"]), sd[p + f"stages.{i}.downsample.1.bias"],
                           stride=2))
        for j in range(depth):
            fused = (cpu_ref._STORE is not None and i == 0 and j == depth - 1
                     and x.shape[2] % 2 == 0 and x.shape[3] % 2 == 0)
            x = cpu_ref.convnext_block(sd, p + f"stages.{i}.blocks.{j}.", x, store=not fused)
            if seg_taps is not None:
                seg_taps[f"s{i}.b{j}"] = None if fused else cpu_ref._rows(x)
        if taps is not None:
            taps[f"stage{i}"] = x
    x = x.mean((2, 3), keepdim=True)
    x = q(cpu_ref._ln2d(x, sd[p + "head.norm.weight"], sd[p + "head.norm.bias"], cpu_ref.LN_EPS_CONVNEXT))
    x = torch.flatten(x, 1)
    if seg_taps is not None:
        seg_taps["pool"] = x
    x = F.linear(x, q(sd[p + "head.fc.weight"]), sd[p + "head.fc.bias"])
    return q(x) if store_out else x


def use_large(monkeypatch):
    """Make cpu_ref's ED / VAE oracles run ConvNeXt-L (inside one test)."""
    monkeypatch.setattr(cpu_ref, "convnext_tiny", convnext_large)


def large_config():
    """The config prediction.py --s large writes (prediction.py:314-318)."""
    from genconvit_amd.model.config import load_config
    cfg = load_config()
    cfg["model"]["backbone"] = "convnext_large"
    cfg["model"]["embedder"] = "swin_large_patch4_window7_224"
    return cfg


_SD = {}


def state_dict(net):
    """Synthetic Large state dicts, one per session: 'ed' (0.8 GB), 'vae' (3.4 GB), 'bb' (the backbone alone)."""
    if net not in _SD:
        if net == "ed":
            _SD[net] = synth.make_state_dict(spec.ed_spec("convnext_large"), synth.DEFAULT_SEED, "edL/")
        elif net == "vae":
            _SD[net] = synth.make_state_dict(spec.vae_spec(True, "convnext_large"), synth.DEFAULT_SEED, "vaeL/")
        else:
            _SD[net] = synth.make_state_dict(spec.convnext_large_spec(""), synth.DEFAULT_SEED, "bbL/")
    return _SD[net]


def hf_convnext_large(sd):
    """Hugging Face ConvNextForImageClassification with Large's widths and depths, loaded with the timm-keyed ``sd``: an
    implementation independent of the oracle (after tests/test_oracle.py::_hf_convnext)."""
    from transformers import ConvNextConfig, ConvNextForImageClassification
    cfg = ConvNextConfig(num_labels=1000, layer_norm_eps=1e-6, hidden_sizes=list(LARGE_DIMS), depths=list(LARGE_DEPTHS))
    m = ConvNextForImageClassification(cfg).eval()
    new = {}
    new["convnext.embeddings.patch_embeddings.weight"] = sd["stem.0.weight"]
    new["convnext.embeddings.patch_embeddings.bias"] = sd["stem.0.bias"]
    new["convnext.embeddings.layernorm.weight"] = sd["stem.1.weight"]
    new["convnext.embeddings.layernorm.bias"] = sd["stem.1.bias"]
    for i, depth in enumerate(LARGE_DEPTHS):
        if i > 0:
            for a in (0, 1):
                for wb in ("weight", "bias"):
                    new[f"convnext.encoder.stages.{i}.downsampling_layer.{a}.{wb}"] = sd[f"stages.{i}.downsample.{a}.{wb}"]
        for j in range(depth):
            s, d = f"stages.{i}.blocks.{j}.", f"convnext.encoder.stages.{i}.layers.{j}."
            new[d + "layer_scale_parameter"] = sd[s + "gamma"]
            for a, b in (("conv_dw", "dwconv"), ("norm", "layernorm"), ("mlp.fc1", "pwconv1"), ("mlp.fc2", "pwconv2")):
                for wb in ("weight", "bias"):
                    new[d + f"{b}.{wb}"] = sd[s + f"{a}.{wb}"]
    new["convnext.layernorm.weight"] = sd["head.norm.weight"]
    new["convnext.layernorm.bias"] = sd["head.norm.bias"]
    new["classifier.weight"] = sd["head.fc.weight"]
    new["classifier.bias"] = sd["head.fc.bias"]
    m.load_state_dict(new, strict=True)
    return m
