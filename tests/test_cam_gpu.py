"""Grad-CAM evidence maps on the MI355X (include/genconvit_hip.h, gcv_*_explain) against the CPU oracle (tests/camutil.py)
fed with the same-dtype oracle's stage-3 tokens (oracle/cpu_ref.py, storage_dtype).

Every case checks these:
- explain's logits are torch.equal to the plain forward's on the same input and eps;
- each pass's maps are within CAM_BOUNDS of the oracle end to end (max |got - want| / rms(want) over the pass's maps);
- they are within TOKEN_BOUNDS of the oracle's head backward applied to the library's own stage-3 tokens;
- the upsampled map is F.interpolate of the raw one.
The oracle is given the library's own decision as its target, so that a near-tie cannot flip the class between the two.
"""
import pytest
import torch

from genconvit_amd import _lib, synth
from oracle import cpu_ref
from tests import camutil
from tests.conftest import synthetic_sd

pytestmark = pytest.mark.gpu
torch.set_grad_enabled(False)

# Bounds: max |Δ| / rms over the maps of one pass, about 3x the largest value one MI355X run measured over the cases
# below (the measured value beside each bound).
# CAM_BOUNDS: against the same-dtype oracle end to end.  The 16-bit stage-3 tokens differ from the oracle's by their storage
# rounding (tests/taputil.py, bb.s3.b).  Through GELU' that stays small.  Through the VAE's ReLU masks it flips whole
# backbone-logit units whose pre-activation is near zero: 14-174 units per case, reported as vae.mask_flips.  Each flip
# moves a frame's map by a sizeable part of its rms, hence the VAE's loose end-to-end bounds.  TOKEN_BOUNDS pins the
# kernels themselves.
CAM_BOUNDS = {
    torch.float32: {"ed.rec": 6.5e-5,                 # 2.12e-05
                    "ed.x": 2.5e-5},                  # 7.60e-06
    torch.float16: {"ed.rec": 8.3e-2,                 # 2.76e-02
                    "ed.x": 2.5e-2,                   # 8.32e-03
                    "vae.x": 1.25,                    # 4.11e-01
                    "vae.xhat": 1.0},                 # 3.20e-01
    torch.bfloat16: {"ed.rec": 0.67,                  # 2.23e-01
                     "ed.x": 0.17,                    # 5.59e-02
                     "vae.x": 2.0,                    # 6.74e-01
                     "vae.xhat": 1.85},               # 6.14e-01
}
# TOKEN_BOUNDS: against the oracle's head backward applied to the library's own stage-3 tokens (tap <net>.bb.s3.b2), with
# the backbone logits and head input rounded where the library stores them: the new kernels' arithmetic.  ED 16-bit:
# one storage rounding of the GELU pre-activations.  VAE fp16 at B = 33 / 128: hidden-layer ReLU units within rounding of
# zero (the other VAE cases measure about 2e-6).
TOKEN_BOUNDS = {
    torch.float32: {"ed.rec": 1.5e-5,                 # 4.94e-06
                    "ed.x": 1.2e-5},                  # 3.85e-06
    torch.float16: {"ed.rec": 6.6e-3,                 # 2.21e-03
                    "ed.x": 4.3e-3,                   # 1.42e-03
                    "vae.x": 0.28,                    # 9.14e-02
                    "vae.xhat": 0.38},                # 1.25e-01
    torch.bfloat16: {"ed.rec": 4.5e-2,                # 1.48e-02
                     "ed.x": 3.4e-2,                  # 1.13e-02
                     "vae.x": 6e-6,                   # 1.97e-06
                     "vae.xhat": 1.2e-5},             # 3.90e-06
}
UP_TOL = 1e-6        # cam224 against F.interpolate of cam_raw, relative to the map's largest value

_HANDLES = {}


def _handle(net, dtype, max_batch=128):
    key = (net, dtype, max_batch)
    if key not in _HANDLES:
        h = _lib.Handle(0, dtype, max_batch)
        if net == "ed":
            h.load_ed(synthetic_sd("ed"))
        else:
            h.load_vae(synthetic_sd("vae"), with_var=False)
        _HANDLES[key] = h
    return _HANDLES[key]


def _oracle_maps(net, dtype, x, eps, merged, target):
    taps = {}
    with cpu_ref.storage_dtype(dtype):
        if net == "ed":
            cpu_ref.ed_forward(synthetic_sd("ed"), x, taps)
        else:
            cpu_ref.vae_forward(synthetic_sd("vae"), x, eps, taps=taps, merged=merged)
    As = camutil.stage3(taps, net, x.shape[0])
    _, cams, _ = camutil.head_cams(synthetic_sd(net), net, As, target, dtype)
    return cams


def _split(net, cam):
    """The library's maps of one network as [(B, hw) per pass]."""
    B = cam.shape[0]
    cam = cam.reshape(B, -1).cpu()
    return [cam[:, :49], cam[:, 49:]]


def _s3_tap(h, net, B, dtype):
    """Tap the library's stage-3 tokens (the tensor the maps are computed from) on handle ``h``."""
    buf = torch.empty(B * sum(camutil.NETS[net][2]) * 768, dtype=dtype, device="cuda")
    h.set_tap(f"{net}.bb.s3.b2", buf)
    return buf


def _check_net(net, dtype, x, eps, merged, logits, cam, up, target, errors, s3_lib):
    """Record the errors of one network's maps (asserted by _assert): against the oracle end to end, and against the
    oracle's head backward applied to the library's own stage-3 tokens (``s3_lib``)."""
    B = x.shape[0]
    t = camutil.resolve_target(target, logits.cpu()) if target is not None else logits.cpu().argmax(1)
    taps = {}
    with cpu_ref.storage_dtype(dtype):
        if net == "ed":
            cpu_ref.ed_forward(synthetic_sd("ed"), x, taps)
        else:
            cpu_ref.vae_forward(synthetic_sd("vae"), x, eps, taps=taps, merged=merged)
    sd = synthetic_sd(net)
    As_ora = camutil.stage3(taps, net, B)
    As_lib = camutil.stage3({f"{net}.bb.s3.b2": s3_lib.cpu()}, net, B)
    _, want, _ = camutil.head_cams(sd, net, As_ora, t, dtype)
    _, same, _ = camutil.head_cams(sd, net, As_lib, t, dtype, as_stored=True)
    got = _split(net, cam)
    for name, g, w, w2 in zip(camutil.PASSES[net], got, want, same):
        errors[name] = camutil.map_error(g, w)
        errors[name + "|tok"] = camutil.map_error(g, w2)
    # backbone-logit units whose activation mask differs between the oracle's stage-3 tokens and the library's
    za, zb = camutil.backbone_logits(sd, net, As_ora, dtype), camutil.backbone_logits(sd, net, As_lib, dtype)
    errors[net + ".mask_flips"] = float(((za > 0) != (zb > 0)).sum())
    if up is not None:
        inp = got[1] if net == "ed" else got[0]
        ref = camutil.upsample(inp, 7)
        errors[net + ".up"] = ((up.cpu() - ref).abs().max() / ref.abs().max().clamp_min(1e-30)).item()


def _assert(dtype, errors):
    bad = []
    for k, v in errors.items():
        if k.endswith(".up"):
            ok = v <= UP_TOL
        elif k.endswith("|tok"):
            ok = v <= TOKEN_BOUNDS[dtype][k[:-4]]
        elif k.endswith(".mask_flips"):
            continue
        else:
            ok = v <= CAM_BOUNDS[dtype][k]
        if not ok:
            bad.append(f"{k} {v:.3e}")
    assert not bad, "out of bounds: " + ", ".join(bad)


def _frames(B, name, dtype):
    x = synth.make_frames(B, name=name)
    eps = synth.make_eps(B, name=name)
    return x, eps, x.to("cuda", dtype), eps.cuda()


def _target_arg(kind, B):
    if kind == "argmax":
        return None
    return torch.tensor([(i * 7 + 3) % 2 for i in range(B)], dtype=torch.int32)


def _report(title, dtype, errors):
    print(f"\n{title}: " + ", ".join(f"{k} {v:.3e}" for k, v in errors.items()))
    _assert(dtype, errors)


@pytest.mark.parametrize("target", ["argmax", "explicit"])
def test_cam_ed_batch32_fp32(target):
    dtype, B = torch.float32, 32
    h = _handle("ed", dtype, 32)
    x, eps, xd, _ = _frames(B, "cam_ed", dtype)
    ref = h.ed_forward(xd)
    t = _target_arg(target, B)
    s3 = _s3_tap(h, "ed", B, dtype)
    try:
        logits, cam, up = h.ed_explain(xd, None if t is None else t.cuda())
        torch.cuda.synchronize()
    finally:
        h.clear_taps()
    assert torch.equal(logits, ref)
    errors = {}
    _check_net("ed", dtype, x, eps, False, logits, cam, up, t, errors, s3)
    _report(f"ED fp32 B={B} {target}", dtype, errors)


@pytest.mark.parametrize("split", [True, False])
def test_cam_vae_batch32_bf16_both_schedules(split, monkeypatch):
    monkeypatch.setenv("GCV_VAE_SPLIT", "1" if split else "0")
    dtype, B = torch.bfloat16, 32
    h = _lib.Handle(0, dtype, 32)          # the schedule switch is read when the handle is created
    h.load_vae(synthetic_sd("vae"), with_var=False)
    try:
        x, eps, xd, ed = _frames(B, "cam_vae", dtype)
        ref = h.vae_forward(xd, ed, want_recon=False)[0]
        s3 = _s3_tap(h, "vae", B, dtype)
        logits, cam, up = h.vae_explain(xd, ed)
        torch.cuda.synchronize()
        assert torch.equal(logits, ref)
        errors = {}
        _check_net("vae", dtype, x, eps, not split, logits, cam, up, None, errors, s3)
    finally:
        h.close()
    _report(f"VAE bf16 B={B} split={split}", dtype, errors)


def _ensemble_case(dtype, B, target, name):
    he, hv = _handle("ed", dtype), _handle("vae", dtype)
    x, eps, xd, ed = _frames(B, name, dtype)
    ref = _lib.genconvit_forward(he, hv, xd, ed)
    t = _target_arg(target, B)
    s3e, s3v = _s3_tap(he, "ed", B, dtype), _s3_tap(hv, "vae", B, dtype)
    try:
        logits, cam_ed, cam_vae, up = _lib.genconvit_explain(he, hv, xd, ed, None if t is None else t.cuda())
        torch.cuda.synchronize()
    finally:
        he.clear_taps()
        hv.clear_taps()
    assert torch.equal(logits, ref)
    errors = {}
    _check_net("ed", dtype, x, eps, True, logits[:B], cam_ed, up[:B], t, errors, s3e)
    _check_net("vae", dtype, x, eps, True, logits[B:], cam_vae, up[B:], t, errors, s3v)
    _report(f"genconvit {dtype} B={B} {target}", dtype, errors)


def test_cam_genconvit_batch128_fp16(monkeypatch):
    monkeypatch.delenv("GCV_VAE_SPLIT", raising=False)
    _ensemble_case(torch.float16, 128, "argmax", "cam_gc")


@pytest.mark.parametrize("target", ["argmax", "explicit"])
@pytest.mark.parametrize("B", [1, 4, 33, 67])
@pytest.mark.parametrize("dtype", [torch.float16, torch.bfloat16], ids=["f16", "bf16"])
def test_cam_genconvit_small_and_odd_batches(dtype, B, target, monkeypatch):
    monkeypatch.delenv("GCV_VAE_SPLIT", raising=False)
    _ensemble_case(dtype, B, target, "cam_odd")


def test_cam_follows_an_occluded_patch():
    """Zeroing the 32 x 32 input patch under the oracle's peak of the original-frame map moves the library's map and the
    oracle's together."""
    dtype = torch.float32
    h = _handle("ed", dtype, 32)
    x, eps, xd, _ = _frames(1, "cam_patch", dtype)
    t = torch.zeros(1, dtype=torch.int32)
    _, cam0, _ = h.ed_explain(xd, t.cuda(), upsample=False)
    want0 = _oracle_maps("ed", dtype, x, eps, False, t)[1]
    k = int(want0[0].argmax())
    i, j = divmod(k, 7)
    x2 = x.clone()
    x2[:, :, 32 * i:32 * i + 32, 32 * j:32 * j + 32] = 0
    _, cam1, _ = h.ed_explain(x2.to("cuda", dtype), t.cuda(), upsample=False)
    want1 = _oracle_maps("ed", dtype, x2, eps, False, t)[1]
    d_got = (cam1 - cam0).reshape(1, -1)[:, 49:].cpu()
    d_want = want1 - want0
    assert d_want.abs().max() > 1e-3 * want0.abs().max()        # the occlusion changes the map
    assert camutil.map_error(d_got, d_want) <= 1e-2
    assert torch.nn.functional.cosine_similarity(d_got, d_want).item() > 0.99


def test_cam_target_changes_the_map():
    dtype, B = torch.float32, 4
    h = _handle("ed", dtype, 32)
    x, eps, xd, _ = _frames(B, "cam_tgt", dtype)
    _, c0, _ = h.ed_explain(xd, torch.zeros(B, dtype=torch.int32, device="cuda"), upsample=False)
    _, c1, _ = h.ed_explain(xd, torch.ones(B, dtype=torch.int32, device="cuda"), upsample=False)
    _, _, a0 = camutil.head_cams(synthetic_sd("ed"), "ed", _stage3("ed", x), 0)
    _, _, a1 = camutil.head_cams(synthetic_sd("ed"), "ed", _stage3("ed", x), 1)
    for p in range(2):
        for b in range(B):
            if not torch.allclose(a0[p][b], a1[p][b]):
                assert not torch.equal(c0[b, p], c1[b, p])


def _stage3(net, x):
    taps = {}
    cpu_ref.ed_forward(synthetic_sd("ed"), x, taps)
    return camutil.stage3(taps, net, x.shape[0])


def test_explain_module_api_matches_forward():
    """GenConViT.explain: the forward's logits (chunking rules included), the cams dict layout, and pred_vid_explain."""
    from genconvit_amd.model.config import load_config
    from genconvit_amd.model.genconvit import GenConViT
    from genconvit_amd.model.genconvit_ed import GenConViTED
    from genconvit_amd.model.genconvit_vae import GenConViTVAE
    from genconvit_amd.model import pred_func
    ed = GenConViTED(load_config(), init="empty")
    ed.load_state_dict(synthetic_sd("ed"))
    vae = GenConViTVAE(load_config(), init="empty")
    vae.load_state_dict(synthetic_sd("vae"), strict=False)
    vae.keep_kl_weights = False
    m = GenConViT.from_modules(ed.cuda().eval(), vae.cuda().eval(), net="genconvit").half()
    B = 15
    x, eps, _, ed_eps = _frames(B, "cam_api", torch.float16)
    ref = m(x.cuda(), eps=ed_eps)
    logits, cams = m.explain(x.cuda(), eps=ed_eps)
    assert torch.equal(logits, ref)
    assert cams["ed"].shape == (B, 2, 7, 7) and cams["vae"].shape == (B, 7, 7) and cams["vae_xhat"].shape == (B, 3, 3)
    assert cams["upsampled"].shape == (2 * B, 224, 224)
    (y, y_val), maps = pred_func.pred_vid_explain(x.cuda(), m)
    assert maps.shape == (2 * B, 224, 224) and maps.min() >= 0 and maps.max() <= 1
    assert y in (0, 1) and 0.0 <= y_val <= 1.0
