"""The stage-2 Grad-CAM oracle (tests/cam2util.py) against autograd through the whole CPU oracle forward, and the public
surface of ``layer`` (header, library exports, Python signatures).

cam2util.s2_cams starts at the stage-2 output and differentiates the down-sampling, stage 3 and the heads only.  Here the
output of stage 2's last block of every pass is caught by wrapping ``cpu_ref.convnext_block``, the full forward runs with
autograd from the input frame at B = 2, and alpha / the maps are formed from those gradients.  The two agree to fp32
rounding, the level tests/test_cam_cpu.py holds its own shortcut to.
"""
import inspect
import os
import re

import pytest
import torch

from genconvit_amd import synth
from oracle import cpu_ref
from tests import cam2util, camutil
from tests.conftest import synthetic_sd

B = 2
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _brute_force(net, sd, monkeypatch, target):
    caught = []
    block = cpu_ref.convnext_block

    def hooked(sd_, p, x, *a, **k):
        y = block(sd_, p, x, *a, **k)
        if p.endswith("stages.2.blocks.8."):
            caught.append(y)
        return y

    monkeypatch.setattr(cpu_ref, "convnext_block", hooked)
    x = synth.make_frames(B, name="cam2cpu").requires_grad_(True)
    taps = {}
    with torch.enable_grad():
        if net == "ed":
            logits = cpu_ref.ed_forward(sd, x, taps)
        else:
            logits = cpu_ref.vae_forward(sd, x, synth.make_eps(B, name="cam2cpu"), taps=taps)[0]
        t = camutil.resolve_target(target, logits)
        grads = torch.autograd.grad(logits.gather(1, t[:, None]).sum(), caught)
    assert len(caught) == 2                                       # both passes, in cat order
    cams, alphas, spread = [], [], 0.0
    for A, g in zip(caught, grads):                               # NCHW
        alpha = g.mean((2, 3))
        spread = max(spread, ((g - alpha[:, :, None, None]).abs().max() / alpha.abs().max()).item())
        alphas.append(alpha)
        cams.append(torch.relu((A.detach() * alpha[:, :, None, None]).sum(1)).flatten(1))
    return logits.detach(), cams, alphas, spread, taps


@pytest.mark.parametrize("target", [None, 0, [1, 0]], ids=["argmax", "class0", "per_frame"])
@pytest.mark.parametrize("net", ["ed", "vae"])
def test_stage2_shortcut_matches_autograd_through_the_oracle(net, target, monkeypatch):
    sd = synthetic_sd(net)
    logits, bf, bf_alpha, spread, taps = _brute_force(net, sd, monkeypatch, target)
    # unlike stage 3, the gradient at the stage-2 map is not uniform over positions: the mean is a real reduction
    assert spread > 1e-2, spread
    got = cam2util.s2_cams(sd, net, cam2util.stage2(taps, net, B), target)
    assert torch.allclose(got["logits"], logits, rtol=1e-5, atol=1e-5)
    assert [tuple(c.shape) for c in got["cams"]] == [(B, s * s) for s in cam2util.SIDES[net]]
    for a, b in zip(got["cams"], bf):
        scale = b.abs().max().clamp_min(1e-30)
        assert ((a - b).abs().max() / scale).item() < 1e-5
    for a, b in zip(got["alphas"], bf_alpha):
        assert ((a - b).abs().max() / b.abs().max()).item() < 1e-5
    assert any(c.abs().max() > 0 for c in got["cams"])           # not a vacuous comparison of zero maps


def test_odd_map_edge_has_zero_gradient():
    """The 7 x 7 stage-2 map of the VAE's 112-pixel pass: its last row and column take no part in the down-sampling."""
    sd = synthetic_sd("vae")
    taps = {}
    cpu_ref.vae_forward(sd, synth.make_frames(B, name="cam2cpu"), synth.make_eps(B, name="cam2cpu"), taps=taps)
    g = cam2util.s2_cams(sd, "vae", cam2util.stage2(taps, "vae", B))["grads"][1]
    assert g.shape[-2:] == (7, 7)
    assert g[:, :, 6, :].abs().max() == 0 and g[:, :, :, 6].abs().max() == 0 and g[:, :, :6, :6].abs().max() > 0


@pytest.mark.parametrize("target", [None, 1], ids=["argmax", "class1"])
@pytest.mark.parametrize("net", ["ed", "vae"])
def test_oracle_meets_head_cams_at_stage3(net, target):
    """Where the two definitions overlap — the maps at the stage-3 output — the new oracle reproduces camutil.head_cams."""
    sd = synthetic_sd(net)
    taps = {}
    x = synth.make_frames(B, name="cam2cpu")
    with torch.no_grad():
        if net == "ed":
            cpu_ref.ed_forward(sd, x, taps)
        else:
            cpu_ref.vae_forward(sd, x, synth.make_eps(B, name="cam2cpu"), taps=taps)
    got = cam2util.s2_cams(sd, net, cam2util.stage2(taps, net, B), target)
    logits, cams, alphas = camutil.head_cams(sd, net, camutil.stage3(taps, net, B), target)
    assert torch.allclose(got["logits"], logits, rtol=1e-5, atol=1e-5)
    for a, b in zip(got["cams3"], cams):
        assert ((a - b).abs().max() / b.abs().max().clamp_min(1e-30)).item() < 1e-5
    for a, b in zip(got["alphas3"], alphas):
        assert ((a - b).abs().max() / b.abs().max()).item() < 1e-5
    assert any(c.abs().max() > 0 for c in cams)


def test_header_declares_and_library_exports_explain_at():
    from genconvit_amd import _lib
    hdr = open(os.path.join(ROOT, "include", "genconvit_hip.h")).read()
    lib = _lib.load()
    for name in ("gcv_ed_explain_at", "gcv_vae_explain_at", "gcv_genconvit_explain_at"):
        m = re.search(r"\bint\s+%s\s*\(([^;]*)\)\s*;" % name, hdr)
        assert m, f"{name} is not declared in include/genconvit_hip.h"
        assert re.search(r"\bint\s+layer\b", m.group(1)), f"{name} takes no layer"
        assert getattr(lib, name) is not None
    # the entries they generalise stay
    for name in ("gcv_ed_explain", "gcv_vae_explain", "gcv_genconvit_explain"):
        assert re.search(r"\bint\s+%s\s*\(" % name, hdr) and getattr(lib, name) is not None


def test_python_explain_takes_layer():
    from genconvit_amd import _lib
    from genconvit_amd.model import pred_func
    from genconvit_amd.model.config import load_config
    from genconvit_amd.model.genconvit import GenConViT
    from genconvit_amd.model.genconvit_ed import GenConViTED
    from genconvit_amd.model.genconvit_vae import GenConViTVAE
    for f in (GenConViT.explain, GenConViTED.explain, GenConViTVAE.explain, pred_func.pred_vid_explain,
              _lib.Handle.ed_explain, _lib.Handle.vae_explain, _lib.genconvit_explain):
        assert inspect.signature(f).parameters["layer"].default == "s3", f
    assert _lib.explain_layer("s3") == (3, False) and _lib.explain_layer("s2") == (2, True)
    ed = GenConViTED(load_config(), init="empty")
    vae = GenConViTVAE(load_config(), init="empty")
    x = synth.make_frames(1)
    for net in ("ed", "vae", "genconvit"):
        m = GenConViT.from_modules(ed, vae, net=net)
        with pytest.raises(ValueError, match="'s3' and 's2'"):
            m.explain(x, layer="nope")
    for m in (ed, vae):
        with pytest.raises(ValueError, match="'s3' and 's2'"):
            m.explain(x, layer="s1")
    with pytest.raises(ValueError, match="'s3' and 's2'"):
        pred_func.pred_vid_explain(x, GenConViT.from_modules(ed, vae, net="genconvit"), layer=None)
