"""ConvNeXt-L backbone (``prediction.py --s large``) on the MI355X: the kernels only Large's shapes reach, the backbone
alone, the ED / VAE / genconvit networks on GCV_CONVNEXT_LARGE handles against the Large restatement of the oracle
(tests/largeutil.py), explain, taps and the batch limits of a Large handle.

16-bit bounds: about 3x what one MI355X run measured (ConvNeXt-L section), beside the delta the CPU restatement
itself predicts between its 16-bit and fp32 evaluations."""
from __future__ import annotations

import ctypes
import math

import pytest
import torch
import torch.nn.functional as F

from genconvit_amd import _lib, synth
from oracle import cpu_ref
from tests import dwcases, kutil, largeutil
from tests.kutil import DTYPES, dev, ptr, rnd, tol

pytestmark = pytest.mark.gpu
ALL = ["f32", "bf16", "f16"]
_KEEP = []


def D(t, dtype=None):
    d = t.to(dev()) if dtype is None else t.to(dev(), dtype)
    _KEEP.append(d)
    if len(_KEEP) > 64:
        torch.cuda.synchronize()
        del _KEEP[:32]
    return d


def q(t, dtype):
    return t.to(dtype).float()


def err(got, want):
    return (got.float().cpu() - want.float()).abs().max().item()


# ----------------------------------------------------------------------------- kernels
@pytest.mark.parametrize("dt", ALL)
@pytest.mark.parametrize("C,H,n", dwcases.LARGE)
def test_dwconv7x7_layernorm_large_shapes(dt, C, H, n):
    """dw 7x7 + LayerNorm at C * W / 7 = 1536 (two channels per lane, dwconv_pair.h) and C = 1536 on maps up to 4 x 4."""
    dtype = DTYPES[dt]
    x = q(rnd((n, C, H, H), 1, 2.0), dtype)
    w = rnd((C, 1, 7, 7), 2, 0.25)
    b, lw, lb = rnd((C,), 3, 0.1), rnd((C,), 4, 0.5) + 1.0, rnd((C,), 5, 0.1)
    want = F.layer_norm(F.conv2d(x, w, b, padding=3, groups=C).permute(0, 2, 3, 1), (C,), lw, lb, 1e-6)
    xd = x.permute(0, 2, 3, 1).contiguous().to(dev(), dtype)
    wdw = w.reshape(C, 49).t().contiguous().to(dev())
    out = torch.full((n + 1, H, H, C), 7.0, dtype=dtype, device=dev())
    kutil.call("gcv_k_dwconv7_ln", _lib.dtype_code(dtype), ptr(xd), ptr(wdw), ptr(D(b)), ptr(D(lw)), ptr(D(lb)), ptr(out),
               n, H, H, C, 1e-6)
    assert (out[n].float() == 7.0).all(), "written beyond the last image"
    assert err(out[:n], want) <= tol(dtype, 3.0)


@pytest.mark.parametrize("dt", ALL)
@pytest.mark.parametrize("layout", ["nchw", "nhwc"])
def test_stem_192_channels(dt, layout):
    dtype = DTYPES[dt]
    n, res, C = 3, 224, 192
    x = q(rnd((n, 3, res, res), 1, 2.0), dtype)
    w = q(rnd((C, 3, 4, 4), 2, 0.2), dtype)
    b, lw, lb = rnd((C,), 3, 0.1), rnd((C,), 4, 0.5) + 1.0, rnd((C,), 5, 0.1)
    want = F.layer_norm(F.conv2d(x, w, b, stride=4).permute(0, 2, 3, 1), (C,), lw, lb, 1e-6)
    wp = w.reshape(C, 48).t().contiguous().to(dev())
    if layout == "nchw":
        xd, st = x.to(dev(), dtype), (3 * res * res, res * res, res, 1)
    else:
        xd, st = x.permute(0, 2, 3, 1).contiguous().to(dev(), dtype), (res * res * 3, 1, res * 3, 3)
    out = torch.zeros((n, res // 4, res // 4, C), dtype=dtype, device=dev())
    kutil.call("gcv_k_stem_ln_c", _lib.dtype_code(dtype), ptr(xd), *st, ptr(wp), ptr(D(b)), ptr(D(lw)), ptr(D(lb)),
               ptr(out), n, res // 4, res // 4, C, 1e-6)
    assert err(out, want) <= tol(dtype, 3.0)


@pytest.mark.parametrize("dt", ALL)
@pytest.mark.parametrize("HW", [49, 9])
def test_pool_layernorm_1536(dt, HW):
    dtype = DTYPES[dt]
    n, C = 5, 1536
    x = q(rnd((n, HW, C), 1, 2.0), dtype)
    lw, lb = rnd((C,), 4, 0.5) + 1.0, rnd((C,), 5, 0.1)
    want = F.layer_norm(x.mean(1), (C,), lw, lb, 1e-6)
    out = torch.zeros((n, C), dtype=dtype, device=dev())
    kutil.call("gcv_k_pool_ln", _lib.dtype_code(dtype), ptr(D(x, dtype)), ptr(D(lw)), ptr(D(lb)), ptr(out), n, HW, C, 1e-6)
    assert err(out, want) <= tol(dtype, 3.0)


@pytest.mark.parametrize("dt", ["bf16", "f16"])
def test_xs192_patchify_epilogue_at_56_pixels(dt):
    """Large stage 0's last block: Xs192 with the LayerNorm-patchify epilogue on 56 x 56 maps (two segments)."""
    dtype, C = DTYPES[dt], 192
    segs = [(3, 56, 56), (2, 56, 56)]
    M = sum(n * h * w for n, h, w in segs)
    x = q(rnd((M, C), 1, 1.5), dtype)
    w1 = q(rnd((4 * C, C), 2, 1 / math.sqrt(C)), dtype)
    w2 = q(rnd((C, 4 * C), 3, 1 / math.sqrt(4 * C)), dtype)
    b1, b2, gamma = rnd((4 * C,), 4, 0.1), rnd((C,), 5, 0.1), rnd((C,), 6, 0.5)
    res = q(rnd((M, C), 7), dtype)
    lw, lb = rnd((C,), 8, 0.5) + 1.0, rnd((C,), 9, 0.1)
    y = res + gamma * (q(F.gelu(x @ w1.t() + b1), dtype) @ w2.t() + b2)
    yn = F.layer_norm(y, (C,), lw, lb, 1e-6)
    want, tok0, hw, wd, out0, t = [], [], [], [], [], 0
    for n, H, W in segs:
        tok0.append(t); hw.append(H * W); wd.append(W); out0.append(t // 4)
        v = yn[t:t + n * H * W].reshape(n, H // 2, 2, W // 2, 2, C).permute(0, 1, 3, 2, 4, 5)
        want.append(v.reshape(n * (H // 2) * (W // 2), 4 * C))
        t += n * H * W
    want = torch.cat(want)
    out = torch.full((M // 4, 4 * C), 7.0, dtype=dtype, device=dev())
    arr = lambda v: (ctypes.c_int * 4)(*(v + [0] * (4 - len(v))))
    kutil.call("gcv_k_fused_mlp_lnp", _lib.dtype_code(dtype), C, ptr(D(x, dtype)), ptr(D(w1, dtype)), ptr(D(b1)),
               ptr(D(w2)), ptr(D(b2)), ptr(D(gamma)), ptr(D(res, dtype)), ptr(D(lw)), ptr(D(lb)), 1e-6, len(segs), arr(tok0),
               arr(hw), arr(wd), arr(out0), ptr(out), M)
    assert err(out, want) <= tol(dtype, 4.0)


@pytest.mark.parametrize("dt", ["bf16", "f16"])
@pytest.mark.parametrize("M", [3 * 784, 64 * 784 + 4 * 784])
def test_pair384_at_28_pixel_token_counts(dt, M):
    """Large stage 1 (C = 384 on 28 x 28 maps): the Pair384 kernels at its token counts."""
    dtype, C = DTYPES[dt], 384
    x = q(rnd((M, C), 1, 1.5), dtype)
    w1 = q(rnd((4 * C, C), 2, 1 / math.sqrt(C)), dtype)
    w2 = q(rnd((C, 4 * C), 3, 1 / math.sqrt(4 * C)), dtype)
    b1, b2, gamma = rnd((4 * C,), 4, 0.1), rnd((C,), 5, 0.1), rnd((C,), 6, 0.5)
    res = q(rnd((M, C), 7), dtype)
    want = res + gamma * (q(F.gelu(x @ w1.t() + b1), dtype) @ w2.t() + b2)
    out = D(res, dtype).clone()
    kutil.call("gcv_k_fused_mlp", _lib.dtype_code(dtype), C, ptr(D(x, dtype)), ptr(D(w1, dtype)), ptr(D(b1)), ptr(D(w2)),
               ptr(D(b2)), ptr(D(gamma)), ptr(out), ptr(out), M)
    assert err(out, want) <= tol(dtype, 2.0)


# ----------------------------------------------------------------------------- networks
def _ed(dtype=torch.float32):
    from genconvit_amd.model.genconvit_ed import GenConViTED
    m = GenConViTED(largeutil.large_config(), init="empty")
    m.load_state_dict(largeutil.state_dict("ed"))
    return m.to(dev(), dtype).eval()


def _vae(dtype=torch.float32):
    from genconvit_amd.model.genconvit_vae import GenConViTVAE
    m = GenConViTVAE(largeutil.large_config(), init="empty")
    m.load_state_dict(largeutil.state_dict("vae"))
    return m.to(dev(), dtype).eval()


def _eps(B, seed=3):
    return torch.randn((B, 12544), generator=torch.Generator().manual_seed(seed))


@pytest.mark.parametrize("res", [224, 112])
def test_backbone_forward_large_fp32(res):
    """gcv_convnext_forward on a Large handle against the fp32 restatement (which tests/test_large_cpu.py pins to HF)."""
    m = _ed()
    x = synth.make_frames(2)
    if res != 224:
        x = F.avg_pool2d(x, 2)
    got = m.backbone_forward(x.to(dev())).float().cpu()
    sd = {k[len("backbone."):]: v for k, v in largeutil.state_dict("ed").items() if k.startswith("backbone.")}
    with torch.no_grad():
        want = largeutil.convnext_large(sd, "", x)
    assert m._get_handle(2).arch == _lib.ARCH_LARGE
    assert err(got, want) <= 1e-3


@pytest.mark.parametrize("res", [32, 64, 96, 128, 156, 224])
def test_backbone_forward_large_fp32_resolutions(res):
    """ConvNeXt-L alone across its resolution range (stage-3 maps 1, 2, 3, 4, 4 and 7 pixels wide: every S of the C = 1536
    whole-map kernel and the band kernel; 156: 39 / 19 / 9 / 4, odd at stages 0 - 2) against the fp32 restatement."""
    m = _ed()
    x = kutil.frames_at(res, 2)
    got = m.backbone_forward(x.to(dev())).float().cpu()
    sd = {k[len("backbone."):]: v for k, v in largeutil.state_dict("ed").items() if k.startswith("backbone.")}
    with torch.no_grad():
        want = largeutil.convnext_large(sd, "", x)
    assert got.shape == want.shape == (2, 1000) and bool(torch.isfinite(got).all())
    e = err(got, want)
    print(f"Large fp32 backbone @{res}: {e:.3e}")
    assert e <= 1e-3


@pytest.mark.parametrize("arch,res,match", [
    ("large", 160, r"multiple of 4 in \[32,156\], or 224, on a ConvNeXt-L handle"),
    ("tiny", 30, r"multiple of 4 in \[32,224\]")])
def test_refused_resolutions_leave_the_handle_as_it_was(arch, res, match):
    """A resolution gcv_convnext_forward does not run is refused with the supported range, before anything is allocated or
    launched: ConvNeXt-L at res 160 (a 5 x 5 stage-3 map, for which C = 1536 has no depthwise kernel), any handle at a res
    that is no multiple of 4.  20 refused calls at the handle's max_batch between two ED forwards on the same handle: the
    second forward is bit-equal to the first.  (Before the refusal moved in front of the pass, a Large pass at res 160
    failed at stage 3 with its token buffers still allocated from the handle's arena — 236 MB per call at 32 fp32 frames,
    by the sizes in run_convnext — and Arena::overflow, once set, was never cleared.  Read from the code; the sequence has
    not been run against the earlier library.)"""
    if arch == "large":
        m = _ed()
    else:
        from genconvit_amd.model.config import load_config
        from genconvit_amd.model.genconvit_ed import GenConViTED
        from tests.conftest import synthetic_sd
        m = GenConViTED(load_config(), init="empty")
        m.load_state_dict(synthetic_sd("ed"))
        m = m.to(dev()).eval()
    x = synth.make_frames(2).to(dev())
    first = m(x).clone()
    h = m._get_handle(2)
    B = h.max_batch
    assert lib_res_ok(h.arch, res) == 0
    bad = F.interpolate(synth.make_frames(B), size=(res, res), mode="bilinear", antialias=True).contiguous().to(dev())
    for _ in range(20):
        with pytest.raises(_lib.GenConViTHipError, match=match):
            m.backbone_forward(bad)
    assert m._get_handle(B) is h, "the refused calls ran on the same handle"
    again = m(x)
    assert torch.equal(first, again)


def lib_res_ok(arch, res):
    return _lib.load().gcv_convnext_res_ok(arch, res)


def test_ed_vae_genconvit_large_fp32(monkeypatch):
    largeutil.use_large(monkeypatch)
    x, eps = synth.make_frames(2), _eps(2)
    ed, vae = _ed(), _vae()
    with torch.no_grad():
        want_ed = cpu_ref.ed_forward(largeutil.state_dict("ed"), x)
        want_vae = cpu_ref.vae_forward(largeutil.state_dict("vae"), x, eps)[0]
    e1 = err(ed(x.to(dev())), want_ed)
    e2 = err(vae(x.to(dev()), eps=eps.to(dev()), want_recon=False)[0], want_vae)
    from genconvit_amd.model.genconvit import GenConViT
    g = GenConViT.from_modules(ed, vae, "genconvit")
    e3 = err(g(x.to(dev()), eps=eps.to(dev())), torch.cat([want_ed, want_vae]))
    print(f"Large fp32 B=2: ED {e1:.2e}  VAE {e2:.2e}  genconvit {e3:.2e}")
    assert max(e1, e2, e3) <= 1e-3


# 16-bit logits bounds (vs the same-dtype restatement, vs the fp32 oracle): about 3x the largest of one MI355X run over
# B = 1, 4, 33 and the B = 128 rows (fp16 1.17e-3 / 7.7e-4, bf16 5.2e-3 / 8.1e-3).  The restatement itself predicts
# 16-bit vs fp32 deltas of 6.2e-4 .. 7.4e-4 (fp16) and 5.1e-3 .. 8.7e-3 (bf16) on these frames.
_B16 = {torch.float16: (3.5e-3, 2.5e-3), torch.bfloat16: (1.5e-2, 2.5e-2)}


@pytest.mark.parametrize("dt", ["f16", "bf16"])
@pytest.mark.parametrize("B", [1, 4, 33])
def test_genconvit_large_16bit(dt, B, monkeypatch):
    dtype = DTYPES[dt]
    largeutil.use_large(monkeypatch)
    rows = sorted({0, B - 1})
    x, eps = synth.make_frames(B), _eps(B)
    ed, vae = _ed(dtype), _vae(dtype)
    from genconvit_amd.model.genconvit import GenConViT
    g = GenConViT.from_modules(ed, vae, "genconvit")
    got = g(x.to(dev(), dtype), eps=eps.to(dev())).float().cpu()
    got = torch.cat([got[:B][rows], got[B:][rows]])
    xs, es = x[rows], eps[rows]
    with torch.no_grad():
        want32 = torch.cat([cpu_ref.ed_forward(largeutil.state_dict("ed"), xs),
                            cpu_ref.vae_forward(largeutil.state_dict("vae"), xs, es)[0]])
        with cpu_ref.storage_dtype(dtype):
            # the restatement's storage points do not depend on the batch (no launch-size rule in the Large path)
            want16 = torch.cat([cpu_ref.ed_forward(largeutil.state_dict("ed"), xs),
                                cpu_ref.vae_forward(largeutil.state_dict("vae"), xs, es)[0]])
    e16, e32, pred = err(got, want16), err(got, want32), err(want16, want32)
    print(f"Large {dt} B={B}: vs same-dtype {e16:.3e}  vs fp32 {e32:.3e}  (restatement 16-bit vs fp32: {pred:.3e})")
    assert e16 <= _B16[dtype][0] and e32 <= _B16[dtype][1]


def test_genconvit_large_fp16_b128_chosen_rows(monkeypatch):
    """B = 128: the first and last frames and both sides of a 32-row tile boundary against the oracle on those frames."""
    largeutil.use_large(monkeypatch)
    B, rows = 128, [0, 31, 32, 127]
    x, eps = synth.make_frames(B), _eps(B)
    from genconvit_amd.model.genconvit import GenConViT
    g = GenConViT.from_modules(_ed(torch.float16), _vae(torch.float16), "genconvit")
    got = g(x.to(dev(), torch.float16), eps=eps.to(dev())).float().cpu()
    got = torch.cat([got[:B][rows], got[B:][rows]])
    with torch.no_grad(), cpu_ref.storage_dtype(torch.float16):
        want = torch.cat([cpu_ref.ed_forward(largeutil.state_dict("ed"), x[rows]),
                          cpu_ref.vae_forward(largeutil.state_dict("vae"), x[rows], eps[rows])[0]])
    e = err(got, want)
    print(f"Large f16 B=128 rows {rows}: vs same-dtype {e:.3e}")
    assert e <= _B16[torch.float16][0]


def _ed_cam_oracle(sd, x, target):
    """Grad-CAM of the ED network by autograd through the fp32 Large restatement's head: maps (B, 2, 7, 7) of the
    [reconstruction, original] passes, ReLU(sum_c dlogit/dA_c(h, w) * A_c(h, w))."""
    with torch.no_grad():
        rec = cpu_ref.ed_decoder(sd, cpu_ref.ed_encoder(sd, x))
        A = []
        for inp in (rec, x):
            taps = {}
            largeutil.convnext_large(sd, "backbone.", inp, taps=taps)
            A.append(taps["stage3"].clone())
    # (autograd on explicitly: other test modules of the suite switch it off process-wide at import)
    with torch.enable_grad():
        A = [a.requires_grad_(True) for a in A]
        feats = []
        for a in A:
            p = cpu_ref._ln2d(a.mean((2, 3), keepdim=True), sd["backbone.head.norm.weight"], sd["backbone.head.norm.bias"],
                              1e-6)
            feats.append(F.linear(torch.flatten(p, 1), sd["backbone.head.fc.weight"], sd["backbone.head.fc.bias"]))
        h = F.gelu(torch.cat(feats, 1))
        logits = F.linear(F.gelu(F.linear(h, sd["fc.weight"], sd["fc.bias"])), sd["fc2.weight"], sd["fc2.bias"])
        logits.gather(1, target.view(-1, 1)).sum().backward()
    return torch.stack([F.relu((a.grad * a).sum(1)) for a in A], 1).detach(), logits.detach()


def test_explain_large_ed_fp32():
    m = _ed()
    x = synth.make_frames(2)
    logits, cams = m.explain(x.to(dev()), upsample=True)
    fwd = m(x.to(dev()))
    assert torch.equal(logits, fwd), "explain's logits must be the forward's"
    target = logits.argmax(1).cpu()
    want, _ = _ed_cam_oracle(largeutil.state_dict("ed"), x, target)
    got = cams["ed"].cpu()
    assert got.shape == (2, 2, 7, 7) and cams["upsampled"].shape == (2, 224, 224)
    rel = err(got, want) / max(want.abs().max().item(), 1e-12)
    print(f"Large ED fp32 explain: max rel map error {rel:.2e}")
    assert rel <= 1e-3


@pytest.mark.parametrize("dt", ["f16"])
def test_explain_large_genconvit_16bit(dt):
    dtype = DTYPES[dt]
    from genconvit_amd.model.genconvit import GenConViT
    g = GenConViT.from_modules(_ed(dtype), _vae(dtype), "genconvit")
    x, eps = synth.make_frames(4), _eps(4)
    logits, cams = g.explain(x.to(dev(), dtype), eps=eps.to(dev()))
    fwd = g(x.to(dev(), dtype), eps=eps.to(dev()))
    assert torch.equal(logits.float(), fwd.float())
    assert cams["ed"].shape == (4, 2, 7, 7) and cams["vae"].shape == (4, 7, 7) and cams["vae_xhat"].shape == (4, 3, 3)
    assert all(torch.isfinite(v).all() and (v >= 0).all() for k, v in cams.items() if v is not None and k != "upsampled")
    # the ED maps against the fp32 oracle's, by correlation (16-bit tokens move the maps by rounding only)
    want, _ = _ed_cam_oracle(largeutil.state_dict("ed"), x, logits[:4].argmax(1).cpu())
    a, b = cams["ed"].float().cpu().flatten(), want.flatten()
    corr = float(torch.corrcoef(torch.stack([a, b]))[0, 1])
    print(f"Large ED {dt} explain: map correlation with the fp32 oracle {corr:.4f}")
    assert corr >= 0.95


def test_taps_large_16bit(monkeypatch):
    dtype = torch.float16
    m = _ed(dtype)
    B = 2
    x = synth.make_frames(B)
    h = m._get_handle(B)
    t_b2 = torch.empty((2 * B * 56 * 56, 192), dtype=dtype, device=dev())
    t_b26 = torch.empty((2 * B * 14 * 14, 768), dtype=dtype, device=dev())
    t_pool = torch.empty((2 * B, 1536), dtype=dtype, device=dev())
    try:
        h.set_tap("ed.bb.s0.b2", t_b2)
        h.set_tap("ed.bb.s2.b26", t_b26)
        h.set_tap("ed.bb.pool", t_pool)
        m(x.to(dev(), dtype))
        torch.cuda.synchronize()
        assert not h.tap_written("ed.bb.s0.b2"), "stage 0's last block goes straight into the patchify epilogue"
        assert h.tap_written("ed.bb.s2.b26") and h.tap_written("ed.bb.pool")
    finally:
        h.clear_taps()
    largeutil.use_large(monkeypatch)
    taps = {}
    with torch.no_grad(), cpu_ref.storage_dtype(dtype):
        cpu_ref.ed_forward(largeutil.state_dict("ed"), x, taps)
    assert taps["ed.bb.s0.b2"] is None
    e1, e2 = err(t_b26, taps["ed.bb.s2.b26"]), err(t_pool, taps["ed.bb.pool"])
    print(f"Large f16 taps: s2.b26 {e1:.3e}  pool {e2:.3e}")
    assert e1 <= 0.06 and e2 <= 0.012            # one MI355X run: 1.95e-2 / 3.9e-3
    with pytest.raises(_lib.GenConViTHipError, match="unknown tap"):
        _lib.Handle(0, torch.float16, 1).set_tap("ed.bb.s2.b26", t_b26)       # Tiny has 9 stage-2 blocks


def test_large_batch_limits():
    lib = _lib.load()
    h = ctypes.c_void_p()
    assert lib.gcv_create_arch(ctypes.byref(h), 0, _lib.dtype_code(torch.float16), 512, _lib.ARCH_LARGE) != 0
    assert "max_batch must be in [1,256] for a ConvNeXt-L handle" in _lib.last_error()
    assert not h
    tiny = _lib.Handle(0, torch.float16, 2)
    large = _lib.Handle(0, torch.float16, 2, _lib.ARCH_LARGE)
    assert (tiny.arch, large.arch) == (_lib.ARCH_TINY, _lib.ARCH_LARGE)
    x = torch.zeros((1, 3, 224, 224), dtype=torch.float16, device=dev())
    eps = torch.zeros((1, 12544), device=dev())
    with pytest.raises(_lib.GenConViTHipError, match="differ in backbone architecture"):
        _lib.genconvit_forward(large, tiny, x, eps)


def test_large_ed_batch_300_equals_chunks():
    m = _ed(torch.float16)
    x = synth.make_frames(300).to(dev(), torch.float16)
    whole = m(x)
    parts = torch.cat([m(x[:256]), m(x[256:])])
    assert m._get_handle(300).max_batch == 256
    assert torch.equal(whole, parts)


def test_load_genconvit_large_checkpoint_and_pred_vid(tmp_path, monkeypatch):
    """prediction.py --s large end to end for net='ed': a published-layout weight file ({'state_dict': ...} with the
    Swin-L embedder keys), load_genconvit, pred_vid against the oracle's vote."""
    from genconvit_amd.model import pred_func
    largeutil.use_large(monkeypatch)
    sd = dict(largeutil.state_dict("ed"))
    sd["embedder.patch_embed.proj.weight"] = torch.zeros(192, 3, 4, 4)
    sd["backbone.patch_embed.proj.weight"] = torch.zeros(1536, 1536, 1, 1)
    monkeypatch.chdir(tmp_path)
    (tmp_path / "weight").mkdir()
    torch.save({"state_dict": sd}, tmp_path / "weight" / "edL.pth")
    model = pred_func.load_genconvit(largeutil.large_config(), "ed", "edL", "unused", False)
    df = synth.make_frames(3)
    y, y_val = pred_func.pred_vid(df, model)
    with torch.no_grad():
        want = cpu_ref.ed_forward(largeutil.state_dict("ed"), df)
    wy, wv = cpu_ref.max_prediction_value(torch.sigmoid(want))
    assert y == wy and abs(y_val - wv) <= 1e-3
