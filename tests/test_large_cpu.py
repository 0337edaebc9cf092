"""ConvNeXt-L backbone (``prediction.py --s large``) on the host side: parameter inventory, construction, the refusal of
other backbones, the Large restatement of the oracle against Hugging Face's ConvNeXt, and the prediction.py alias with
the --s large config rewrite.  No GPU needed."""
from __future__ import annotations

import math
import os
import sys

import pytest
import torch

from genconvit_amd import _lib, spec, synth
from oracle import cpu_ref
from tests import largeutil


def _numel(entries):
    return sum(math.prod(s) for _, s, _ in entries)


def test_convnext_large_spec_matches_timm_inventory():
    """timm 0.6.5 convnext_large: 197 767 336 parameters, Tiny's key layout with the wider shapes and 27 stage-2 blocks."""
    sp = spec.convnext_large_spec("")
    assert _numel(sp) == 197_767_336
    shapes = {n: s for n, s, _ in sp}
    assert shapes["stem.0.weight"] == (192, 3, 4, 4) and shapes["stem.1.weight"] == (192,)
    assert shapes["stages.2.blocks.26.mlp.fc1.weight"] == (3072, 768)
    assert "stages.2.blocks.27.gamma" not in shapes
    assert shapes["stages.3.downsample.1.weight"] == (1536, 768, 2, 2)
    assert shapes["stages.3.blocks.2.mlp.fc2.weight"] == (1536, 6144)
    assert shapes["head.norm.weight"] == (1536,) and shapes["head.fc.weight"] == (1000, 1536)
    # the same key set as Tiny's for the blocks both have, in the same order
    tiny = [n for n, _, _ in spec.convnext_tiny_spec("")]
    large = [n for n, _, _ in sp]
    assert [n for n in large if n in set(tiny)] == tiny
    assert set(large) - set(tiny) == {f"stages.2.blocks.{j}.{k}" for j in range(9, 27)
                                      for k in ("conv_dw.weight", "conv_dw.bias", "norm.weight", "norm.bias",
                                                "mlp.fc1.weight", "mlp.fc1.bias", "mlp.fc2.weight", "mlp.fc2.bias", "gamma")}


def test_tiny_spec_unchanged():
    assert _numel(spec.convnext_tiny_spec("")) == 28_589_128
    assert spec.ed_spec() == spec.ed_spec("convnext_tiny")
    assert spec.vae_spec() == spec.vae_spec(True, "convnext_tiny")


@pytest.mark.parametrize("net", ["ed", "vae"])
def test_large_network_state_dict_layout(net):
    from genconvit_amd.model.genconvit_ed import GenConViTED
    from genconvit_amd.model.genconvit_vae import GenConViTVAE
    cls, sp, prefix = ((GenConViTED, spec.ed_spec("convnext_large"), "backbone.") if net == "ed"
                       else (GenConViTVAE, spec.vae_spec(True, "convnext_large"), "convnext_backbone."))
    m = cls(largeutil.large_config(), init="empty")
    sd = m.state_dict()
    assert set(sd) == {n for n, _, _ in sp} and len(sd) == len(sp)
    assert all(tuple(sd[n].shape) == s for n, s, _ in sp)
    assert tuple(sd[prefix + "stages.2.blocks.26.mlp.fc2.weight"].shape) == (768, 3072)
    assert m.backbone_name == "convnext_large" and m._arch == _lib.ARCH_LARGE and m._cap == 256
    # the published checkpoints also hold the Swin-L embedder: accepted and ignored, as for Tiny
    extra = dict(sd)
    extra["embedder.patch_embed.proj.weight"] = torch.zeros(192, 3, 4, 4)
    extra[prefix + "patch_embed.proj.weight"] = torch.zeros(1536, 1536, 1, 1)
    m.load_state_dict(extra)


def test_large_genconvit_constructs_and_has_no_cpu_fallback(tmp_path, monkeypatch):
    from genconvit_amd.model.genconvit import GenConViT
    from genconvit_amd.model.genconvit_ed import GenConViTED
    monkeypatch.chdir(tmp_path)
    (tmp_path / "weight").mkdir()
    m = GenConViTED(largeutil.large_config(), init="empty")
    torch.save({"state_dict": m.state_dict()}, tmp_path / "weight" / "edL.pth")
    g = GenConViT(largeutil.large_config(), "edL", "none", "ed", False)
    assert g.model_ed.backbone_name == "convnext_large"
    with pytest.raises(_lib.GenConViTHipError, match="no CPU fallback"):
        g(torch.zeros(1, 3, 224, 224))


@pytest.mark.parametrize("name", ["convnext_small", "convnext_base", "swin_tiny"])
def test_other_backbones_still_raise(name):
    from genconvit_amd.model.config import load_config
    from genconvit_amd.model.genconvit_ed import GenConViTED
    from genconvit_amd.model.genconvit_vae import GenConViTVAE
    cfg = load_config()
    cfg["model"]["backbone"] = name
    for cls in (GenConViTED, GenConViTVAE):
        with pytest.raises(ValueError, match="convnext_tiny.*convnext_large"):
            cls(cfg, init="empty")


def test_large_chunks_at_256():
    from genconvit_amd.model.genconvit_ed import GenConViTED
    m = GenConViTED(largeutil.large_config(), init="empty")
    assert m._chunks(300) == [(0, 256), (256, 300)]
    assert m.reserve(1000)._max_batch == 256


@pytest.mark.parametrize("res", [224, 112])
def test_large_restatement_vs_huggingface(res):
    """The Large restatement (tests/largeutil.py) against Hugging Face's independent ConvNeXt at Large's widths."""
    pytest.importorskip("transformers")
    sd = largeutil.state_dict("bb")
    m = largeutil.hf_convnext_large(sd)
    x = synth.make_frames(2)
    if res != 224:
        x = torch.nn.functional.avg_pool2d(x, 2)
    with torch.no_grad():
        ours = largeutil.convnext_large(sd, "", x)
        theirs = m(pixel_values=x).logits
    assert float((ours - theirs).abs().max()) < 5e-5


def test_large_restatement_storage_points():
    """16-bit: only the last stage-0 block (Xs192's LayerNorm-patchify epilogue, even maps) skips its store; stage 1
    keeps every block (Pair384 has no epilogue); fp32 stores every block."""
    sd = largeutil.state_dict("bb")
    x = synth.make_frames(1)
    for dt, none_keys in ((torch.float16, {"s0.b2"}), (torch.float32, set())):
        seg = {}
        with cpu_ref.storage_dtype(dt), torch.no_grad():
            largeutil.convnext_large(sd, "", x, seg_taps=seg)
        assert {k for k, v in seg.items() if v is None} == none_keys
        assert seg["s2.b26"].shape == (14 * 14, 768) and seg["pool"].shape == (1, 1536)


def test_prediction_alias_large_config_constructs(tmp_path, monkeypatch):
    """prediction.py --s large on the ``model`` alias: load_config, the backbone / embedder rewrite of prediction.py:314-318,
    then load_genconvit from cwd-relative weight files in the published layout."""
    import genconvit_amd.model as gm
    names = ("config", "genconvit", "genconvit_ed", "genconvit_vae", "model_embedder", "pred_func")
    saved = {k: sys.modules.get(k) for k in ["model"] + [f"model.{n}" for n in names]}
    try:
        sys.modules["model"] = gm
        for n in names:
            sys.modules[f"model.{n}"] = __import__(f"genconvit_amd.model.{n}", fromlist=["_"])
        monkeypatch.chdir(tmp_path)
        (tmp_path / "weight").mkdir()
        from genconvit_amd.model.genconvit_ed import GenConViTED
        sd = GenConViTED(largeutil.large_config(), init="empty").state_dict()
        sd["embedder.patch_embed.proj.weight"] = torch.zeros(192, 3, 4, 4)
        torch.save({"state_dict": sd}, tmp_path / "weight" / "ed_large.pth")
        pred = {}
        exec("from model.pred_func import *\nfrom model.config import load_config\n", pred)
        config = pred["load_config"]()
        config["model"]["backbone"] = "convnext_large"                       # prediction.py:314-318
        config["model"]["embedder"] = "swin_large_patch4_window7_224"
        model = pred["load_genconvit"](config, "ed", "ed_large", "unused", False)
        assert model.model_ed.backbone_name == "convnext_large" and not model.training
        assert os.path.isfile(tmp_path / "weight" / "ed_large.pth")
    finally:
        for k, m in saved.items():
            if m is None:
                sys.modules.pop(k, None)
            else:
                sys.modules[k] = m
