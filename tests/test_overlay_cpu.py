"""The heat overlay without a GPU: the colour map, the exported entry, the CPU restatement of the kernel's arithmetic
(tests/overlayutil.py) against F.interpolate and against values worked out by hand, and the argument checks of
``_lib.cam_overlay`` and ``pred_func.explain_frames``, which all run before anything is launched."""
import os
import re

import pytest
import torch
import torch.nn.functional as F

from genconvit_amd import _lib
from genconvit_amd.model import pred_func
from tests import overlayutil as ou

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
torch.set_grad_enabled(False)


def _rand_frames(shape, seed):
    g = torch.Generator().manual_seed(seed)
    return torch.randint(0, 256, shape, dtype=torch.uint8, generator=g)


def _rand_maps(shape, seed):
    return torch.rand(shape, generator=torch.Generator().manual_seed(seed))


# ----------------------------------------------------------------------------- colour map and ABI
def test_jet_lut_matches_the_restatement():
    lut = _lib.jet_lut()
    assert lut.dtype == torch.uint8 and tuple(lut.shape) == (256, 3)
    assert torch.equal(lut, ou.jet_lut_ref())
    assert lut[0].tolist() == [0, 0, 128] and lut[255].tolist() == [128, 0, 0]      # blue end, red end
    assert lut[128].tolist()[1] == 255                                               # green in the middle


def test_header_declares_and_library_exports_gcv_cam_overlay():
    hdr = open(os.path.join(REPO, "include", "genconvit_hip.h")).read()
    assert re.search(r"\bint\s+gcv_cam_overlay\s*\(", hdr)
    assert "gcv_cam_overlay" in _lib.SIGNATURES
    assert hasattr(_lib.load(), "gcv_cam_overlay")


# ----------------------------------------------------------------------------- sampling
@pytest.mark.parametrize("m", [1, 3, 7, 14, 224])
def test_sample_ref_is_bilinear_interpolation(m):
    """sample_ref against F.interpolate(mode="bilinear", align_corners=False) evaluated in float64: values in [0, 1] and a
    handful of fp32 roundings stay below 1e-6, so 1e-5 is slack."""
    M = _rand_maps((m, m), 100 + m)
    sides = [1, 2, 3, 5, 6, 7, 13, 14, 15, 27, 28, 100, 223, 224, 225, 399, 448, 700]
    worst = 0.0
    for h, w in [(s, s) for s in sides] + [(1, 700), (700, 1), (3, 224), (450, 37), (37, 450), (224, 7)]:
        got = ou.sample_ref(M, h, w)
        want = F.interpolate(M.double()[None, None], size=(h, w), mode="bilinear", align_corners=False)[0, 0]
        assert got.dtype == torch.float32 and got.shape == (h, w)
        worst = max(worst, (got.double() - want).abs().max().item())
    print(f"\nmap {m}x{m}: max |sample_ref - interpolate| = {worst:.3e}")
    assert worst <= 1e-5


def test_sample_ref_non_square_map_and_clamp():
    M = _rand_maps((7, 14), 5)
    got = ou.sample_ref(M, 90, 61)
    want = F.interpolate(M.double()[None, None], size=(90, 61), mode="bilinear", align_corners=False)[0, 0]
    assert (got.double() - want).abs().max().item() <= 1e-5
    v = ou.sample_ref(torch.tensor([[-1.0, 2.0]]), 1, 2)
    assert v.tolist() == [[0.0, 1.0]]                             # values are taken as [0, 1]


# ----------------------------------------------------------------------------- properties of overlay_ref
def _scene(seed=0):
    frames = _rand_frames((3, 40, 53, 3), seed)
    boxes = [(0, 2, 30, 20, 5), (0, 10, 50, 35, 22), (2, 0, 53, 40, 0)]        # two overlapping on frame 0, frame 1 bare
    maps = _rand_maps((3, 7, 7), seed + 1)
    return frames, boxes, maps


def _outside_mask(frames, boxes):
    m = torch.ones(frames.shape[:3], dtype=torch.bool)
    for f, t, r, b, l in boxes:
        m[f, t:b, l:r] = False
    return m


@pytest.mark.parametrize("weighted", [True, False])
def test_pixels_outside_every_box_are_unchanged(weighted):
    frames, boxes, maps = _scene()
    out = ou.overlay_ref(frames, boxes, maps, 0.5, weighted)
    m = _outside_mask(frames, boxes)
    assert torch.equal(out[m], frames[m])
    assert torch.equal(out[1], frames[1])
    assert not torch.equal(out[0], frames[0]) and not torch.equal(out[2], frames[2])


@pytest.mark.parametrize("weighted", [True, False])
def test_alpha_zero_is_the_identity(weighted):
    frames, boxes, maps = _scene(3)
    assert torch.equal(ou.overlay_ref(frames, boxes, maps, 0.0, weighted), frames)


def test_alpha_one_flat_gives_the_lut_colour():
    frames = _rand_frames((1, 30, 31, 3), 7)
    maps = _rand_maps((1, 3, 3), 8)
    lut = _rand_frames((256, 3), 9)
    out = ou.overlay_ref(frames, [(0, 0, 31, 30, 0)], maps, 1.0, False, lut)
    k = torch.round(ou.sample_ref(maps[0], 30, 31) * 255.0).long()
    assert torch.equal(out[0], lut[k])


def test_weighted_leaves_cold_pixels_unchanged():
    frames = _rand_frames((1, 20, 20, 3), 11)
    maps = torch.zeros((1, 2, 2))
    maps[0, :, 1] = 1.0                                           # cold left, hot right
    out = ou.overlay_ref(frames, [(0, 0, 20, 20, 0)], maps, 1.0, True)
    v = ou.sample_ref(maps[0], 20, 20)
    hot = v > 0.999                                               # k = 255 and a8 = rint(256 v) = 256
    assert (v == 0).any() and hot.any()
    assert torch.equal(out[0][v == 0], frames[0][v == 0])
    assert torch.equal(out[0][hot], ou.jet_lut_ref()[255].expand(int(hot.sum()), 3))
    flat = ou.overlay_ref(frames, [(0, 0, 20, 20, 0)], maps, 1.0, False)
    assert torch.equal(flat[0][v == 0], ou.jet_lut_ref()[0].expand(int((v == 0).sum()), 3))


def test_later_box_wins_in_the_overlap():
    frames = _rand_frames((1, 32, 32, 3), 13)
    a, b = (0, 0, 20, 20, 0), (0, 10, 32, 32, 10)
    maps = torch.stack((torch.zeros(4, 4), torch.ones(4, 4)))
    lut = ou.jet_lut_ref()
    ab = ou.overlay_ref(frames, [a, b], maps, 1.0, False)
    ba = ou.overlay_ref(frames, [b, a], maps.flip(0), 1.0, False)
    assert torch.equal(ab[0, 10:20, 10:20], lut[255].expand(10, 10, 3))
    assert torch.equal(ba[0, 10:20, 10:20], lut[0].expand(10, 10, 3))
    assert torch.equal(ab[0, :10, :20], lut[0].expand(10, 20, 3))
    # at alpha < 1 the later box is blended over what the earlier one left
    half = ou.overlay_ref(frames, [a, b], maps, 0.5, False)
    first = ou.overlay_ref(frames, [a], maps[:1], 0.5, False)
    assert torch.equal(half, ou.overlay_ref(first, [b], maps[1:], 0.5, False))


def test_blend_values_worked_by_hand():
    lut = torch.zeros((256, 3), dtype=torch.uint8)
    lut[:, 0] = torch.arange(256, dtype=torch.uint8)              # lut[k] = (k, 0, 255)
    lut[:, 2] = 255
    frames = torch.tensor([[[[100, 200, 50]]]], dtype=torch.uint8)
    one = lambda v, alpha, weighted: ou.overlay_ref(frames, [(0, 0, 1, 1, 0)], torch.tensor([[[v]]]), alpha, weighted,
                                                    lut)[0, 0, 0].tolist()
    # v = 1: k = 255; alpha 0.5 -> a8 = 128: (100 * 128 + 255 * 128 + 128) >> 8 = 178; (200 * 128 + 128) >> 8 = 100;
    # (50 * 128 + 255 * 128 + 128) >> 8 = 153
    assert one(1.0, 0.5, False) == [178, 100, 153]
    assert one(1.0, 0.5, True) == [178, 100, 153]
    # v = 0.5: k = rint(127.5) = 128 (half to even); weighted a8 = rint(64) = 64:
    # (100 * 192 + 128 * 64 + 128) >> 8 = 107; (200 * 192 + 128) >> 8 = 150; (50 * 192 + 255 * 64 + 128) >> 8 = 101
    assert one(0.5, 0.5, True) == [107, 150, 101]
    # flat: a8 = 128: (100 * 128 + 128 * 128 + 128) >> 8 = 114
    assert one(0.5, 0.5, False) == [114, 100, 153]
    # alpha 1 flat: exactly the colour; alpha 0.3 -> a8 = rint(76.8) = 77: (100 * 179 + 255 * 77 + 128) >> 8 = 147
    assert one(1.0, 1.0, False) == [255, 0, 255]
    assert one(1.0, 0.3, False) == [147, (200 * 179 + 128) >> 8, (50 * 179 + 255 * 77 + 128) >> 8]
    # a 2 x 1 map over a 4-row box: rows sample at (2j + 1) 2 - 4 over 8 = 0 (clamped), 1/4, 3/4, 1 (second tap clamped)
    v = ou.sample_ref(torch.tensor([[0.0], [1.0]]), 4, 1)[:, 0].tolist()
    assert v == [0.0, 0.25, 0.75, 1.0]


# ----------------------------------------------------------------------------- argument checks (before any launch)
def test_cam_overlay_rejects_bad_input():
    frames = _rand_frames((2, 20, 30, 3), 1)
    maps = _rand_maps((1, 7, 7), 2)
    box = [(0, 2, 12, 12, 2)]
    E = _lib.GenConViTHipError
    with pytest.raises(E, match="frames"):                        # host tensors: there is no CPU path
        _lib.cam_overlay(frames, box, maps)
    with pytest.raises(E, match="frames"):
        _lib.cam_overlay(frames.float(), box, maps)
    with pytest.raises(E, match="frames"):
        _lib.cam_overlay(frames[..., :2], box, maps)
    with pytest.raises(E, match="box 1 lies outside"):
        _lib.cam_overlay(frames, box + [(0, 2, 31, 12, 2)], maps.expand(2, 7, 7))
    with pytest.raises(E, match="box 0 lies outside"):
        _lib.cam_overlay(frames, [(2, 2, 12, 12, 2)], maps)
    with pytest.raises(E, match="maps holds 1 maps for 2 boxes"):
        _lib.cam_overlay(frames, box + box, maps)
    with pytest.raises(E, match="maps"):
        _lib.cam_overlay(frames, box, maps[0])
    with pytest.raises(E, match="maps"):
        _lib.cam_overlay(frames, box, torch.zeros((1, 7, 7), dtype=torch.int32))
    with pytest.raises(E, match="maps"):
        _lib.cam_overlay(frames, box, torch.zeros((1, 225, 7)))
    for alpha in (-0.01, 1.01, float("nan")):
        with pytest.raises(E, match="alpha"):
            _lib.cam_overlay(frames, box, maps, alpha=alpha)
    with pytest.raises(E, match="lut"):
        _lib.cam_overlay(frames, box, maps, lut=torch.zeros((256, 4), dtype=torch.uint8))
    with pytest.raises(E, match="lut"):
        _lib.cam_overlay(frames, box, maps, lut=torch.zeros((256, 3)))


class _NoModel:
    """A model that must not be reached."""
    net = "genconvit"

    def parameters(self):
        raise AssertionError("the model was used")

    def explain(self, *a, **k):
        raise AssertionError("the model was used")


def test_explain_frames_rejects_bad_input():
    frames = _rand_frames((2, 20, 30, 3), 1)
    box = [(0, 2, 12, 12, 2)]
    with pytest.raises(ValueError, match="unknown map 'both'"):
        pred_func.explain_frames(frames, _NoModel(), boxes=box, which="both")
    with pytest.raises(_lib.GenConViTHipError, match="box 0 lies outside"):
        pred_func.explain_frames(frames.numpy(), _NoModel(), boxes=[(0, 2, 31, 12, 2)])
    with pytest.raises(_lib.GenConViTHipError, match="box 1 lies outside"):
        pred_func.explain_frames(frames, _NoModel(), locate=lambda fr: box + [(1, 12, 12, 12, 2)])
    with pytest.raises(_lib.GenConViTHipError, match="frames"):
        pred_func.explain_frames(frames.float(), _NoModel(), boxes=box)


def test_explain_frames_without_a_face_runs_nothing():
    frames = _rand_frames((2, 20, 30, 3), 1)
    (y, y_val), overlays, boxes = pred_func.explain_frames(frames.numpy(), _NoModel(), locate=lambda fr: [])
    assert y is None and y_val is None and boxes == []
    assert overlays.dtype == torch.uint8 and torch.equal(overlays.cpu(), frames)
