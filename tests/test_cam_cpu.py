"""The Grad-CAM oracle (tests/camutil.py) against autograd through the whole CPU oracle forward.

camutil.head_cams uses the shortcut the kernels implement: average pooling makes d logit / d A the same at every position
of the stage-3 map, so only the heads need a backward.  Here the last ConvNeXt block's output of every pass is caught by
wrapping ``cpu_ref.convnext_block`` (a forward hook on the functional oracle), the full forward runs with autograd at B = 2,
and Grad-CAM is formed from the real per-position gradients.  The two agree to fp32 rounding.
"""
import pytest
import torch

from genconvit_amd import synth
from oracle import cpu_ref
from tests import camutil
from tests.conftest import synthetic_sd

B = 2


def _brute_force(net, sd, monkeypatch, target):
    caught = []
    block = cpu_ref.convnext_block

    def hooked(sd_, p, x, *a, **k):
        y = block(sd_, p, x, *a, **k)
        if p.endswith("stages.3.blocks.2."):
            caught.append(y)
        return y

    monkeypatch.setattr(cpu_ref, "convnext_block", hooked)
    x = synth.make_frames(B, name="camcpu").requires_grad_(True)
    taps = {}
    with torch.enable_grad():
        if net == "ed":
            logits = cpu_ref.ed_forward(sd, x, taps)
        else:
            logits = cpu_ref.vae_forward(sd, x, synth.make_eps(B, name="camcpu"), taps=taps)[0]
        t = camutil.resolve_target(target, logits)
        grads = torch.autograd.grad(logits.gather(1, t[:, None]).sum(), caught)
    assert len(caught) == 2                                       # both passes, in cat order
    cams, spread = [], 0.0
    for A, g in zip(caught, grads):                               # NCHW
        alpha = g.mean((2, 3))
        spread = max(spread, ((g - alpha[:, :, None, None]).abs().max() / alpha.abs().max()).item())
        cams.append(torch.relu((A.detach() * alpha[:, :, None, None]).sum(1)).flatten(1))
    return logits.detach(), cams, spread, taps


@pytest.mark.parametrize("target", [None, 0, [1, 0]], ids=["argmax", "class0", "per_frame"])
@pytest.mark.parametrize("net", ["ed", "vae"])
def test_shortcut_matches_autograd_through_the_oracle(net, target, monkeypatch):
    sd = synthetic_sd(net)
    logits, bf, spread, taps = _brute_force(net, sd, monkeypatch, target)
    # the gradient at the stage-3 map is uniform over positions up to fp32 rounding
    assert spread < 1e-5, spread
    got_logits, cams, _ = camutil.head_cams(sd, net, camutil.stage3(taps, net, B), target)
    assert torch.allclose(got_logits, logits, rtol=1e-5, atol=1e-5)
    for a, b in zip(cams, bf):
        scale = b.abs().max().clamp_min(1e-30)
        assert ((a - b).abs().max() / scale).item() < 1e-5
    assert any(c.abs().max() > 0 for c in cams)                  # not a vacuous comparison of zero maps


def test_targets_give_different_maps():
    """The two classes' maps differ whenever their Grad-CAM weights do."""
    sd = synthetic_sd("ed")
    taps = {}
    cpu_ref.ed_forward(sd, synth.make_frames(B, name="camcpu"), taps)
    As = camutil.stage3(taps, "ed", B)
    _, c0, a0 = camutil.head_cams(sd, "ed", As, 0)
    _, c1, a1 = camutil.head_cams(sd, "ed", As, 1)
    for p in range(2):
        assert not torch.allclose(a0[p], a1[p])
        assert not torch.equal(c0[p], c1[p])

