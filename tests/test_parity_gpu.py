"""End-to-end parity on the MI355X: the HIP path (through the host mirror classes -> ctypes -> C ABI)
against (a) the committed golden vectors produced by the reference's own classes
(tests/golden/make_golden.py) and (b) the CPU oracle on the same seeded inputs.

Tolerance: north_star's "logits within 1e-3 of the reference PyTorch CPU path" for fp32 storage.
16-bit storage (bf16 / fp16, "--fp16" of the reference) is reported against the fp32 oracle with the
looser bound written in each test.
"""
import numpy as np
import pytest
import torch

from genconvit_amd import _lib, synth
from genconvit_amd.model.config import load_config
from genconvit_amd.model.genconvit import GenConViT
from genconvit_amd.model.genconvit_ed import GenConViTED
from genconvit_amd.model.genconvit_vae import GenConViTVAE
from genconvit_amd.model import pred_func
from oracle import cpu_ref

pytestmark = pytest.mark.gpu
torch.set_grad_enabled(False)

FP32_TOL = 1e-3          # north_star
_CACHE = {}


def slice64(t):
    f = t.detach().float().cpu().flatten()
    idx = torch.linspace(0, f.numel() - 1, 64).long()
    return f[idx].numpy()


def ed_model(dtype=torch.float32):
    key = ("ed", dtype)
    if key not in _CACHE:
        m = GenConViTED(load_config(), init="empty")
        from tests.conftest import synthetic_sd
        m.load_state_dict(synthetic_sd("ed"))
        _CACHE[key] = m.to("cuda").to(dtype).eval()
    return _CACHE[key]


def vae_model(dtype=torch.float32):
    key = ("vae", dtype)
    if key not in _CACHE:
        m = GenConViTVAE(load_config(), init="empty")
        from tests.conftest import synthetic_sd
        m.load_state_dict(synthetic_sd("vae"))
        _CACHE[key] = m.to("cuda").to(dtype).eval()
    return _CACHE[key]


def fresh_vae(dtype, split, monkeypatch):
    """A VAE model on a NEW handle created under GCV_VAE_SPLIT=<split>: the library reads the switch when a handle is
    constructed (net_impl.h), so the two schedules of gcv_vae_forward — backbone(x) forked to a side stream, or one
    merged two-segment pass on the caller's stream (what --no-concurrent, every profiled step and profiles/*serial*
    run) — are both reachable from one test process."""
    from tests.conftest import synthetic_sd
    monkeypatch.setenv("GCV_VAE_SPLIT", "1" if split else "0")
    m = GenConViTVAE(load_config(), init="empty")
    m.load_state_dict(synthetic_sd("vae"))
    return m.to("cuda").to(dtype).eval()


# ----------------------------------------------------------------------------- fp32: the parity gate
def test_ed_fp32_matches_reference_golden(golden, sd_ed):
    x = synth.make_frames(4)
    got = ed_model()(x.cuda()).cpu()
    err_gold = np.abs(got.numpy() - golden["ed_logits"]).max()
    err_orc = (got - cpu_ref.ed_forward(sd_ed, x)).abs().max().item()
    print(f"\nED fp32 B=4: |logits - reference golden| = {err_gold:.3e}, vs oracle = {err_orc:.3e}")
    assert err_gold <= FP32_TOL and err_orc <= FP32_TOL


@pytest.mark.parametrize("res", [224, 112])
def test_convnext_fp32_matches_oracle(res, sd_ed, hf_golden):
    """ConvNeXt-T alone, against the oracle's restatement AND against the committed outputs of the independent
    Hugging Face implementation (tests/golden/make_hf_golden.py) — numbers that never went through cpu_ref's backbone."""
    x = synth.make_frames(3, name=f"cnx{res}")
    if res != 224:
        x = torch.nn.functional.avg_pool2d(x, 224 // res)
    got = ed_model().backbone_forward(x.cuda()).cpu()
    want = cpu_ref.convnext_tiny(sd_ed, "backbone.", x)
    err = (got - want).abs().max().item()
    err_hf = np.abs(got.numpy() - hf_golden[f"cnx{res}"]).max()
    print(f"\nConvNeXt-T fp32 @{res}: max |logits1000 diff| = {err:.3e} vs oracle, {err_hf:.3e} vs Hugging Face "
          f"(|want| max {want.abs().max():.2f})")
    assert err <= FP32_TOL and err_hf <= FP32_TOL


# gcv_convnext_forward takes every multiple of 4 in [32, 224]: 49 resolutions.  Their maps are res / 4 pixels wide, halved with
# floor per stage, so the sweep runs every depthwise kernel a ConvNeXt-T pass can reach (the generic tile kernel wherever the
# width is not 7 NS, the whole-map kernel of 1 x 1 ... 4 x 4 stage-3 maps), odd maps at every stage (last row / column
# dropped by the down-sampling) and the MLP / GEMM kernels from 1 token per frame up.
CNX_RES = list(range(32, 228, 4))
# 16-bit: a subset that touches each arm.  stage widths: 32: 8/4/2/1, 36: 9/4/2/1 (odd stage 0), 56: 14/7/3/1 (Tile at
# C = 96, Roll, Tiny 3, 1), 64: 16/8/4/2, 96: 24/12/6/3, 100: 25/12/6/3, 128: 32/16/8/4, 160: 40/20/10/5 (Tile at every
# stage), 196: 49/24/12/6, 220: 55/27/13/6 (odd at stages 0 - 2: the un-fused LayerNorm-patchify), 224: 56/28/14/7
CNX_RES_16 = [32, 36, 56, 64, 96, 100, 128, 160, 196, 220, 224]
# max |logits1000 - same-dtype restatement| over 3 frames, one MI355X run, per resolution of CNX_RES_16 in that order:
#   fp16: 6.35e-03 6.73e-03 5.86e-03 4.39e-03 3.91e-03 3.91e-03 3.91e-03 3.91e-03 3.91e-03 3.91e-03 2.93e-03
#   bf16: 4.10e-02 5.08e-02 4.69e-02 3.12e-02 3.12e-02 3.12e-02 3.12e-02 3.12e-02 3.12e-02 3.12e-02 2.34e-02
# Bound: about 3x the largest (the suite's convention, tests/taputil.py): 6.73e-3 (fp16) and 5.08e-2 (bf16), both at res 36.
# The logits are stored in the 16-bit dtype and reach |4.8|; one ulp there is 3.906e-3 (fp16) / 3.125e-2 (bf16), and half of
# that below 4.  Res 96 ... 220 differ from the restatement by exactly one such ulp (a logit on a rounding boundary going
# the other way), 224 (all |logits| < 4) by 1.5 ulp of the lower binade.  Res 32 ... 56 come to 1.5 - 1.7 ulp, 2.3x the
# value at 224: their stage-3 map is a single token, so the pooled feature carries one token's rounding error instead of
# the mean over up to 49, and the restatement's own 16-bit vs fp32 delta — no HIP kernel in it — grows the same way
# (fp16 4.4e-3 ... 5.0e-3 at 32 ... 56 against 2.9e-3 at 224; bf16 3.7e-2 against 2.0e-2).
CNX_BOUND_16 = {torch.float16: 2e-2, torch.bfloat16: 1.5e-1}


@pytest.mark.parametrize("res", CNX_RES)
def test_convnext_fp32_every_resolution(res, sd_ed):
    """ConvNeXt-T alone, fp32, at every resolution gcv_convnext_forward accepts, against the oracle: all 3 x 1000 logits."""
    from tests import kutil
    x = kutil.frames_at(res, 3)
    got = ed_model().backbone_forward(x.cuda()).cpu()
    want = cpu_ref.convnext_tiny(sd_ed, "backbone.", x)
    assert got.shape == want.shape == (3, 1000) and bool(torch.isfinite(got).all())
    err = (got - want).abs().max().item()
    print(f"\nConvNeXt-T fp32 @{res}: max |logits1000 diff| = {err:.3e} (|want| max {want.abs().max():.2f})")
    assert err <= FP32_TOL


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16])
@pytest.mark.parametrize("res", CNX_RES_16)
def test_convnext_16bit_resolutions_vs_same_dtype_restatement(dtype, res, sd_ed):
    """ConvNeXt-T alone in 16-bit storage against the oracle's same-dtype restatement (cpu_ref.storage_dtype: the CPU
    evaluation rounded where the HIP path stores, with the even / odd map and fused-epilogue rules), all 3 x 1000 logits."""
    from tests import kutil
    x = kutil.frames_at(res, 3).to(dtype).float()
    got = ed_model(dtype).backbone_forward(x.cuda()).float().cpu()
    with cpu_ref.storage_dtype(dtype):
        want = cpu_ref.convnext_tiny(sd_ed, "backbone.", x)
    want32 = cpu_ref.convnext_tiny(sd_ed, "backbone.", x)
    assert got.shape == want.shape == (3, 1000) and bool(torch.isfinite(got).all())
    err = (got - want).abs().max().item()
    print(f"\nConvNeXt-T {dtype} @{res}: max |logits1000 - same-dtype restatement| = {err:.3e} "
          f"(restatement vs fp32 oracle {(want - want32).abs().max():.3e}, |want| max {want.abs().max():.2f})")
    assert err <= CNX_BOUND_16[dtype]


def test_ed_vae_fp32_match_huggingface_backed_golden(golden, hf_golden):
    """ED / VAE logits with the backbone evaluated by the independent implementation (the glue around it is the
    reference's own, pinned bit-exact): the HIP path is within 1e-3 of numbers no line of cpu_ref's ConvNeXt produced."""
    x = synth.make_frames(4)
    eps = torch.from_numpy(golden["vae_eps"])
    e_ed = np.abs(ed_model()(x.cuda()).cpu().numpy() - hf_golden["ed_logits_hf"]).max()
    e_vae = np.abs(vae_model()(x.cuda(), eps=eps.cuda(), want_recon=False)[0].cpu().numpy() - hf_golden["vae_logits_hf"]).max()
    print(f"\nfp32 B=4 vs Hugging-Face-backed golden: ed {e_ed:.3e}, vae {e_vae:.3e}")
    assert e_ed <= FP32_TOL and e_vae <= FP32_TOL


def test_vae_fp32_matches_reference_golden(golden, sd_vae):
    x = synth.make_frames(4)
    eps = torch.from_numpy(golden["vae_eps"])
    m = vae_model()
    logits, recon = m(x.cuda(), eps=eps.cuda(), want_recon=True, want_mse=True, want_kl=True)
    err_gold = np.abs(logits.cpu().numpy() - golden["vae_logits"]).max()
    print(f"\nVAE fp32 B=4: |logits - reference golden| = {err_gold:.3e}")
    assert err_gold <= FP32_TOL
    assert np.abs(slice64(recon) - golden["vae_recon_slice"]).max() <= 1e-3
    assert np.abs(m.mse.cpu().numpy() - golden["vae_mse"]).max() <= 1e-3 * golden["vae_mse"].max()
    assert abs(float(m.kl) - float(golden["vae_kl"])) <= 1e-4 * abs(float(golden["vae_kl"]))
    assert recon.shape == (4, 3, 224, 224)


def test_genconvit_concat_and_vote_match_reference_golden(golden):
    x = synth.make_frames(4)
    eps = torch.from_numpy(golden["vae_eps"])
    g = GenConViT.from_modules(ed_model(), vae_model(), net="genconvit")
    out = g(x.cuda(), eps=eps.cuda())
    assert out.shape == (8, 2)                                  # cat((ed, vae), dim=0), model/genconvit.py:74
    assert np.abs(out.cpu().numpy() - golden["genconvit_logits"]).max() <= FP32_TOL
    y, val = pred_func.max_prediction_value(torch.sigmoid(out.squeeze()))
    assert y == int(golden["vote_idx"]) and abs(val - float(golden["vote_val"])) <= 1e-3
    assert pred_func.real_or_fake(y) == str(golden["vote_label"])
    dv = _lib.vote(out).cpu()                                   # device-side K15
    assert abs(float(dv[y]) - torch.sigmoid(out).mean(0)[y].item()) <= 1e-6
    for net, rows in (("ed", 4), ("vae", 4)):
        o = GenConViT.from_modules(ed_model(), vae_model(), net=net)(x.cuda(), eps=eps.cuda())
        assert o.shape == (rows, 2)
        ref = golden["ed_logits"] if net == "ed" else golden["vae_logits"]
        assert np.abs(o.cpu().numpy() - ref).max() <= FP32_TOL


def test_pred_vid_drop_in(golden):
    """pred_vid(df, model) of model/pred_func.py:111-120 on CPU frames with the VAE eps pinned."""
    x = synth.make_frames(4)
    eps = torch.from_numpy(golden["vae_eps"]).cuda()
    g = GenConViT.from_modules(ed_model(), vae_model(), net="genconvit")
    fwd = g.forward
    g.forward = lambda df: fwd(df, eps=eps)          # pin the RNG draw for the check
    y, val = pred_func.pred_vid(x, g)                # x on CPU: moved to the model device like the reference
    assert y == int(golden["vote_idx"]) and abs(val - float(golden["vote_val"])) <= 1e-3


# ----------------------------------------------------------------------------- edge cases / properties
def test_batch_of_one_and_ragged_batches(sd_ed):
    x = synth.make_frames(7, name="ragged")
    m = ed_model()
    full = m(x.cuda()).cpu()
    one = m(x[:1].cuda()).cpu()
    assert one.shape == (1, 2)
    assert (one - full[:1]).abs().max().item() <= 1e-5
    parts = torch.cat([m(x[0:3].cuda()).cpu(), m(x[3:7].cuda()).cpu()])
    assert (parts - full).abs().max().item() <= 1e-5           # frames are independent (shardable)
    assert (full - cpu_ref.ed_forward(sd_ed, x)).abs().max().item() <= FP32_TOL


def test_empty_batch_gives_empty_logits():
    """The reference's nn.Modules accept a (0,3,224,224) batch; pred_vid never sends one (`len(df) >= 1`)."""
    x = torch.zeros((0, 3, 224, 224))
    assert ed_model()(x.cuda()).shape == (0, 2)
    lo, rec = vae_model()(x.cuda())
    assert lo.shape == (0, 2) and rec.shape == (0, 3, 224, 224)
    g = GenConViT.from_modules(ed_model(), vae_model(), net="genconvit")
    assert g(x.cuda()).shape == (0, 2)
    assert pred_func.pred_vids([x, synth.make_frames(2, name="e")], g)[0] is None


def test_shards_reassemble_to_unsharded_result(golden):
    """§8e: 8 shards run one after the other on one GPU == the unsharded (2B,2) tensor."""
    from genconvit_amd import dist as gdist
    B, world = 11, 8
    x = synth.make_frames(B, name="shard").cuda()
    eps = synth.make_eps(B).cuda()
    g = GenConViT.from_modules(ed_model(), vae_model(), net="genconvit")
    full = g(x, eps=eps).cpu()
    ed_rows, vae_rows = [], []
    for r in range(world):
        lo, hi = gdist.shard_bounds(B, world, r)
        if hi == lo:
            continue
        o = g(x[lo:hi], eps=eps[lo:hi]).cpu()
        ed_rows.append(o[:hi - lo])
        vae_rows.append(o[hi - lo:])
    re = torch.cat(ed_rows + vae_rows)
    assert re.shape == full.shape and (re - full).abs().max().item() <= 1e-5


def test_full_size_config2_ed_batch32_fp32(sd_ed):
    """BASELINE.json configs[1]: ed, batch 32, fp32 — every frame against the oracle."""
    x = synth.make_frames(32, name="cfg2")
    got = ed_model()(x.cuda()).cpu()
    want = cpu_ref.ed_forward(sd_ed, x)
    err = (got - want).abs().max().item()
    print(f"\nED fp32 B=32: max |logits diff| = {err:.3e}")
    assert err <= FP32_TOL and torch.isfinite(got).all()


def test_input_dtype_and_device_are_normalised():
    x = synth.make_frames(2)
    m = ed_model()
    a = m(x.cuda())
    b = m(x.double())            # CPU + wrong dtype: moved / cast at the boundary
    assert (a - b).abs().max().item() <= 1e-6


def test_missing_weight_key_is_an_error():
    from tests.conftest import synthetic_sd
    sd = dict(synthetic_sd("ed"))
    sd.pop("backbone.stages.2.blocks.4.gamma")
    h = _lib.Handle(0, torch.float32, 2)
    with pytest.raises(_lib.GenConViTHipError, match="missing weight tensor 'backbone.stages.2.blocks.4.gamma'"):
        h.load_ed(sd)
    with pytest.raises(_lib.GenConViTHipError, match="not loaded"):
        h.ed_forward(torch.zeros(1, 3, 224, 224, device="cuda"))
    h.close()


# ----------------------------------------------------------------------------- 16-bit storage
# Bounds = about 3x what was measured on the MI355X (fp16 6e-4 / 4e-4, bf16 5e-3 / 1e-2 for ed / vae at B=4), against
# BOTH the fp32 reference golden and the same-dtype CPU restatement (oracle with weights and activations rounded at
# the HIP path's storage points): a 10x regression cannot pass.
BOUND_16 = {torch.float16: 2e-3, torch.bfloat16: 3e-2}
# The yardstick the reference itself sets: its own --fp16 pipeline (model.half() on .half() frames, model/genconvit.py:24-25,
# 59-61; every op in torch.float16, and the same for bfloat16) deviates from its fp32 run by 9.3e-4 / 6.8e-4 (ed / vae, fp16)
# and 7.8e-3 / 5.6e-3 (bf16) on these frames (tests/golden/make_golden.py, keys *_logits_half / *_logits_bf16).  The HIP
# path's 16-bit storage must stay within twice that.
REF_16 = {torch.float16: "half", torch.bfloat16: "bf16"}


def _reference_16bit_delta(golden, net, dtype):
    return float(np.abs(golden[f"{net}_logits_{REF_16[dtype]}"] - golden[f"{net}_logits"]).max())


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16])
def test_ed_16bit_delta_vs_fp32_oracle_and_same_dtype_restatement(dtype, golden, sd_ed):
    x = synth.make_frames(4)
    got = ed_model(dtype)(x.cuda()).cpu()
    err = np.abs(got.numpy() - golden["ed_logits"]).max()
    with cpu_ref.storage_dtype(dtype):
        same = cpu_ref.ed_forward(sd_ed, x)
    err_same = (got - same).abs().max().item()
    pred = np.abs(same.numpy() - golden["ed_logits"]).max()
    ref16 = _reference_16bit_delta(golden, "ed", dtype)
    print(f"\nED {dtype} B=4: |logits - fp32 reference golden| = {err:.3e}; vs same-dtype restatement {err_same:.3e} "
          f"(restatement vs fp32: {pred:.3e}); the reference's own {REF_16[dtype]} run vs its fp32 run: {ref16:.3e}")
    assert err <= BOUND_16[dtype] and err_same <= BOUND_16[dtype]
    assert err <= 2.0 * ref16, "16-bit storage deviates more than twice what the reference's own 16-bit pipeline does"


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16])
def test_vae_16bit_delta_vs_fp32_oracle_and_same_dtype_restatement(dtype, golden, sd_vae):
    x = synth.make_frames(4)
    eps = torch.from_numpy(golden["vae_eps"])
    logits, _ = vae_model(dtype)(x.cuda(), eps=eps.cuda(), want_recon=False)
    got = logits.cpu()
    err = np.abs(got.numpy() - golden["vae_logits"]).max()
    with cpu_ref.storage_dtype(dtype):
        same = cpu_ref.vae_forward(sd_vae, x, eps)[0]
    err_same = (got - same).abs().max().item()
    ref16 = _reference_16bit_delta(golden, "vae", dtype)
    print(f"\nVAE {dtype} B=4: |logits - fp32 reference golden| = {err:.3e}; vs same-dtype restatement {err_same:.3e}; "
          f"the reference's own {REF_16[dtype]} run vs its fp32 run: {ref16:.3e}")
    assert err <= BOUND_16[dtype] and err_same <= BOUND_16[dtype]
    assert err <= 2.0 * ref16, "16-bit storage deviates more than twice what the reference's own 16-bit pipeline does"


@pytest.mark.parametrize("split", [False, True])
def test_vae_both_schedules_fp32_golden_and_bf16_batch32(split, golden, sd_vae, monkeypatch):
    """Both schedules of gcv_vae_forward (see fresh_vae) against the reference golden at fp32 and, at configs[2]'s size,
    against the fp32 oracle at bf16; the two schedules must also agree with each other bit for bit (same kernels, same
    order per stream)."""
    x = synth.make_frames(4)
    eps = torch.from_numpy(golden["vae_eps"])
    m = fresh_vae(torch.float32, split, monkeypatch)
    logits, recon = m(x.cuda(), eps=eps.cuda(), want_recon=True, want_mse=True, want_kl=True)
    err_gold = np.abs(logits.cpu().numpy() - golden["vae_logits"]).max()
    assert err_gold <= FP32_TOL
    assert np.abs(slice64(recon) - golden["vae_recon_slice"]).max() <= 1e-3
    assert np.abs(m.mse.cpu().numpy() - golden["vae_mse"]).max() <= 1e-3 * golden["vae_mse"].max()
    ref = vae_model()(x.cuda(), eps=eps.cuda(), want_recon=False)[0]          # the cached model: default schedule
    assert torch.equal(logits, ref), "the split and the merged VAE schedule must give identical logits"
    del m
    xb = synth.make_frames(32, name="cfg3")
    eb = synth.make_eps(32, name="cfg3")
    mb = fresh_vae(torch.bfloat16, split, monkeypatch)
    got = mb(xb.cuda(), eps=eb.cuda(), want_recon=False)[0].cpu()
    want = cpu_ref.vae_forward(sd_vae, xb, eb)[0]
    err = (got - want).abs().max().item()
    print(f"\nVAE split={split}: fp32 B=4 vs golden {err_gold:.3e}; bf16 B=32 vs fp32 oracle {err:.3e}")
    assert got.shape == (32, 2) and torch.isfinite(got).all() and err <= 5e-2


def test_full_size_config3_vae_batch32_bf16(sd_vae):
    """BASELINE.json configs[2]: vae, batch 32, bf16 — at its stated size (M = 125 440 tokens at stage 0 takes the
    LDS-resident fused MLP and the 128-byte-row DMA ring, which B=4 never reaches): every frame against the fp32
    oracle and the bf16 restatement, eps fixed."""
    x = synth.make_frames(32, name="cfg3")
    eps = synth.make_eps(32, name="cfg3")
    got = vae_model(torch.bfloat16)(x.cuda(), eps=eps.cuda(), want_recon=False)[0].cpu()
    want = cpu_ref.vae_forward(sd_vae, x, eps)[0]
    with cpu_ref.storage_dtype(torch.bfloat16):
        same = cpu_ref.vae_forward(sd_vae, x, eps)[0]
    err, err_same = (got - want).abs().max().item(), (got - same).abs().max().item()
    print(f"\nVAE bf16 B=32: max |logits - fp32 oracle| = {err:.3e}, vs bf16 restatement {err_same:.3e}")
    assert got.shape == (32, 2) and torch.isfinite(got).all()
    assert err <= 5e-2 and err_same <= 5e-2


@pytest.mark.parametrize("B", [33, 67])
def test_odd_batches_16bit_against_the_fp32_path(B):
    """Odd image counts in 16-bit storage: the 112-pixel segment of the VAE's merged pass then holds 784 B tokens, which is not
    a multiple of the 32-token wave tiles, so tiles straddle the segment boundary in the MLP kernels whose epilogue applies the
    stage boundary's LayerNorm + space-to-depth per segment (fused_mlp_res.h, xs_mlp.h); B = 67 also runs the matrix-pipe
    dw kernel with ragged 19-row bands.  Checked against the fp32 path of the same library (itself within 2e-6 of the oracle
    at B = 32), frame by frame."""
    x = synth.make_frames(B, name="odd")
    eps = synth.make_eps(B, name="odd").cuda()
    ref = GenConViT.from_modules(ed_model(), vae_model(), net="genconvit")(x.cuda(), eps=eps).float().cpu()
    for dtype, bound in ((torch.float16, 4e-3), (torch.bfloat16, 5e-2)):
        g = GenConViT.from_modules(ed_model(dtype), vae_model(dtype), net="genconvit")
        got = g(x.cuda(), eps=eps).float().cpu()
        err = (got - ref).abs().max().item()
        print(f"\ngenconvit {dtype} B={B}: all rows vs the fp32 path: {err:.2e}")
        assert got.shape == (2 * B, 2) and torch.isfinite(got).all() and err <= bound


# ----------------------------------------------------------------------------- Swin-T embedder (row A6)
def test_full_size_config4_genconvit_batch128_fp16(golden):
    """BASELINE.json configs[3]: genconvit, batch 128, fp16 — the batch size at which the large-M kernels run
    (LDS-resident fused MLP, 128-byte-row LDS-DMA GEMM).  Frames are independent, so rows of the B=128 result must
    agree with the same frames pushed through as a batch of 4 (other kernels, other tile shapes), and the first four
    frames with the reference's fp32 golden within the fp16 bound."""
    x = synth.make_frames(128, name="frames")
    x4 = synth.make_frames(4)
    eps = torch.cat([torch.from_numpy(golden["vae_eps"]), synth.make_eps(124, name="cfg4")]).cuda()
    assert torch.equal(x[:4], x4), "synthetic frames are index-addressed"
    g = GenConViT.from_modules(ed_model(torch.float16), vae_model(torch.float16), net="genconvit")
    big = g(x.cuda(), eps=eps).float().cpu()
    assert big.shape == (256, 2) and torch.isfinite(big).all()
    small = g(x4.cuda(), eps=eps[:4]).float().cpu()
    d_ed = (big[0:4] - small[0:4]).abs().max().item()
    d_vae = (big[128:132] - small[4:8]).abs().max().item()
    e_ed = np.abs(big[0:4].numpy() - golden["ed_logits"]).max()
    e_vae = np.abs(big[128:132].numpy() - golden["vae_logits"]).max()
    print(f"\ngenconvit fp16 B=128: rows vs B=4 run: ed {d_ed:.2e} vae {d_vae:.2e}; vs fp32 golden: ed {e_ed:.2e} vae {e_vae:.2e}")
    assert d_ed <= 2e-3 and d_vae <= 2e-3
    assert e_ed <= 2e-3 and e_vae <= 2e-3
    # every one of the 128 frames against the fp32 CPU oracle (about 10 s of host time)
    from tests.conftest import synthetic_sd
    want = cpu_ref.genconvit_forward(synthetic_sd("ed"), synthetic_sd("vae"), x, eps.cpu())
    e_all = (big - want).abs().max().item()
    print(f"genconvit fp16 B=128: all 256 rows vs fp32 oracle: {e_all:.2e}")
    assert e_all <= 4e-3
    # shards of 32 reassemble to the same rows (the multi-GPU partition, run back to back on one GPU)
    parts = [g(x[i:i + 32].cuda(), eps=eps[i:i + 32]).float().cpu() for i in range(0, 128, 32)]
    re = torch.cat([torch.cat([p[:32] for p in parts]), torch.cat([p[32:] for p in parts])])
    assert (re - big).abs().max().item() <= 2e-3


def swin_model(dtype=torch.float32):
    key = ("swin", dtype)
    if key not in _CACHE:
        from genconvit_amd import spec
        from genconvit_amd.model.swin import SwinTinyEmbedder
        m = SwinTinyEmbedder(init="empty")
        m.load_state_dict(synth.make_state_dict(spec.swin_tiny_spec(""), synth.DEFAULT_SEED, "swin/"))
        _CACHE[key] = m.to("cuda").to(dtype).eval()
        _CACHE[("swin_sd",)] = {k: v.float().cpu() for k, v in m.state_dict().items()} if dtype == torch.float32 else None
    return _CACHE[key]


def test_swin_tiny_fp32_matches_oracle(hf_golden):
    """timm swin_tiny_patch4_window7_224 forward (W-MSA/SW-MSA, rel-pos bias, patch merging) vs the
    CPU restatement (itself cross-checked against Hugging Face Swin in tests/test_oracle.py)."""
    from genconvit_amd import spec
    sd = synth.make_state_dict(spec.swin_tiny_spec(""), synth.DEFAULT_SEED, "swin/")
    x = synth.make_frames(3, name="swin")
    got = swin_model()(x.cuda()).cpu()
    want = cpu_ref.swin_tiny(sd, "", x)
    err = (got - want).abs().max().item()
    err_hf = np.abs(got.numpy() - hf_golden["swin"]).max()
    print(f"\nSwin-T fp32: max |logits1000 diff| = {err:.3e} vs oracle, {err_hf:.3e} vs Hugging Face "
          f"(|want| max {want.abs().max():.2f})")
    assert err <= FP32_TOL and err_hf <= FP32_TOL


def test_hybrid_embed_probe_runs_swin_on_the_gpu():
    """HybridEmbed.__init__ (model/model_embedder.py:16-37): one Swin forward on zeros(1,3,224,224)
    to read the dims -> grid (1,1000), proj Conv2d(1000,768,1)."""
    from genconvit_amd.model.model_embedder import HybridEmbed
    he = HybridEmbed(swin_model(), img_size=224, embed_dim=768)
    assert he.grid_size == (1, 1000) and tuple(he.proj.weight.shape) == (768, 1000, 1, 1)


@pytest.mark.parametrize("dtype,bound", [(torch.bfloat16, 9e-2), (torch.float16, 1.2e-2)])   # 3x the measured 3.0e-2 / 3.9e-3
def test_swin_tiny_16bit_delta(dtype, bound):
    from genconvit_amd import spec
    sd = synth.make_state_dict(spec.swin_tiny_spec(""), synth.DEFAULT_SEED, "swin/")
    x = synth.make_frames(2, name="swin")
    got = swin_model(dtype)(x.cuda()).float().cpu()
    err = (got - cpu_ref.swin_tiny(sd, "", x)).abs().max().item()
    print(f"\nSwin-T {dtype}: max |logits1000 diff vs fp32 oracle| = {err:.3e}")
    assert err <= bound


# ----------------------------------------------------------------------------- row N3: several videos per forward
def test_pred_vids_batches_videos_and_votes_per_video():
    """One forward over the concatenated crops of several videos + per-video device vote == pred_vid per video."""
    lens = [4, 1, 6, 0, 3]
    total = sum(lens)
    eps_all = synth.make_eps(total, name="n3").cuda()
    x = synth.make_frames(total, name="n3")
    g = GenConViT.from_modules(ed_model(), vae_model(), net="genconvit")
    fwd = g.forward
    state = {"o": 0}

    def pinned(df):                      # frame f always sees eps_all[f], batched or not
        o = state["o"]
        state["o"] += df.shape[0]
        return fwd(df, eps=eps_all[o:o + df.shape[0]])
    g.forward = pinned
    dfs, o = [], 0
    for n in lens:
        dfs.append(x[o:o + n])
        o += n
    want = [pred_func.pred_vid(d, g) if len(d) else None for d in dfs]
    for max_batch in (128, 5):           # one forward for all / groups split at video boundaries
        state["o"] = 0
        got = pred_func.pred_vids(dfs, g, max_batch=max_batch)
        assert got[3] is None
        for gv, wv in zip(got, want):
            if wv is not None:
                assert gv[0] == wv[0] and abs(gv[1] - wv[1]) <= 1e-5
    g1 = GenConViT.from_modules(ed_model(), None, net="ed")
    got = pred_func.pred_vids([dfs[0], dfs[2]], g1)
    for gv, d in zip(got, (dfs[0], dfs[2])):
        wv = pred_func.pred_vid(d, g1)
        assert gv[0] == wv[0] and abs(gv[1] - wv[1]) <= 1e-5


# ----------------------------------------------------------------------------- rows A14 / N2: load_genconvit from files
def _published_layout(sd, which):
    """The key layout of the published checkpoints: the path's tensors plus the Swin
    embedder registered twice, HybridEmbed.proj and the BatchNorm counters — wrapped as {'state_dict': ...}."""
    from genconvit_amd import spec
    out = dict(sd)
    swin = synth.make_state_dict(spec.swin_tiny_spec(""), synth.DEFAULT_SEED, "swin/")
    bb = "backbone." if which == "ed" else "convnext_backbone."
    for k, v in swin.items():
        out["embedder." + k] = v
        out[bb + "patch_embed.backbone." + k] = v
    out[bb + "patch_embed.proj.weight"] = torch.zeros(768, 1000, 1, 1)
    out[bb + "patch_embed.proj.bias"] = torch.zeros(768)
    if which == "vae":
        for i in (1, 4, 7, 10):
            out[f"encoder.features.{i}.num_batches_tracked"] = torch.tensor(0)
    return {"epoch": 29, "state_dict": out, "min_loss": 0.1}


@pytest.fixture(scope="module")
def weight_dir(tmp_path_factory):
    from tests.conftest import synthetic_sd
    d = tmp_path_factory.mktemp("gcv_weights")
    (d / "weight").mkdir()
    torch.save(_published_layout(synthetic_sd("ed"), "ed"), d / "weight" / "genconvit_ed_inference.pth")
    torch.save(_published_layout(synthetic_sd("vae"), "vae"), d / "weight" / "genconvit_vae_inference.pth")
    return d


@pytest.mark.parametrize("fp16", [False, True])
def test_load_genconvit_and_pred_vid_from_published_layout_files(weight_dir, monkeypatch, golden, fp16):
    """model/pred_func.py:18-64 + :111-120 end to end on the GPU: load_genconvit(config, net, ed, vae, fp16) reads
    weight/{name}.pth (full-size files in the published layout, both Swin copies and the {'state_dict': ...}
    wrapper included), pred_vid votes.  Also row N2: what the load leaves on the device."""
    from tests.conftest import synthetic_sd
    monkeypatch.chdir(weight_dir)                                  # weight/ is resolved against the cwd (genconvit.py:16)
    torch.cuda.synchronize()
    free0 = torch.cuda.mem_get_info()[0]
    model = pred_func.load_genconvit(load_config(), "genconvit", "genconvit_ed_inference", "genconvit_vae_inference", fp16)
    assert next(model.parameters()).is_cuda                       # pred_vid's device discovery (:114)
    assert model.model_vae.encoder.mu.weight.device.type == "cpu"  # the 1.26 GB matrices stay host-resident
    x = synth.make_frames(4)
    seed = 1234
    g = torch.Generator(device="cuda"); g.manual_seed(seed)
    model.model_vae.set_generator(g)
    y, val = pred_func.pred_vid(x, model)
    torch.cuda.synchronize()
    torch.cuda.empty_cache()                                       # (count what is held, not the allocator's free blocks)
    used = (free0 - torch.cuda.mem_get_info()[0]) / 2**30
    g2 = torch.Generator(device="cuda"); g2.manual_seed(seed)
    eps = torch.randn((4, 12544), dtype=torch.float32, device="cuda", generator=g2).cpu()
    want = cpu_ref.genconvit_forward(synthetic_sd("ed"), synthetic_sd("vae"), x, eps)
    wy, wval = cpu_ref.vote(want)
    print(f"\nload_genconvit(fp16={fp16}) + pred_vid: ({y}, {val:.5f}) vs oracle ({wy}, {wval:.5f}); device memory in use "
          f"after load + one forward: {used:.2f} GiB (packed weights + two B<=32 workspaces; the fp32 nn.Parameters alone "
          f"would be 2.8 GiB, round 1 held them plus 2.4-2.6 GiB of packed copies)")
    assert y == wy and abs(val - wval) <= (2e-3 if fp16 else 1e-4)
    assert used < (2.0 if fp16 else 3.0)
    sd = model.state_dict()
    assert "model_vae.encoder.mu.weight" in sd and sd["model_vae.encoder.mu.weight"].shape == (12544, 25088)
    with pytest.raises(_lib.GenConViTHipError, match="encoder.var"):
        model.model_vae(x.cuda(), want_kl=True)                   # inference wrapper leaves encoder.var unpacked


def test_reference_logits_dtype_opt_in(golden):
    """model/genconvit.py:59-61: after .half() the reference's logits are fp16; the mirror returns fp32 unless
    GenConViT.reference_logits_dtype is set, then exactly the fp32 logits rounded to the model dtype."""
    x = synth.make_frames(4).cuda()
    eps = torch.from_numpy(golden["vae_eps"]).cuda()
    g = GenConViT.from_modules(ed_model(torch.float16), vae_model(torch.float16), net="genconvit")
    a = g(x, eps=eps)
    try:
        GenConViT.reference_logits_dtype = True
        b = g(x, eps=eps)
    finally:
        GenConViT.reference_logits_dtype = False
    assert a.dtype == torch.float32 and b.dtype == torch.float16 and torch.equal(a.half(), b)
    y = pred_func.max_prediction_value(b)          # the vote accepts the reference's fp16 logits as well
    assert y[0] in (0, 1)


# ----------------------------------------------------------------------------- C boundary: ensemble entry point, RCCL
def test_genconvit_forward_entry_point_equals_the_two_separate_forwards(golden):
    """gcv_genconvit_forward (model/genconvit.py:66-75 behind one C call: ED and VAE on two internal streams, joined with
    events) returns exactly what gcv_ed_forward + gcv_vae_forward + cat return."""
    x = synth.make_frames(6, name="ens").cuda()
    eps = synth.make_eps(6, name="ens").cuda()
    g = GenConViT.from_modules(ed_model(), vae_model(), net="genconvit")
    try:
        GenConViT.concurrent = True
        a = g(x, eps=eps)
        b = g(x, eps=eps)
        GenConViT.concurrent = False
        c = g(x, eps=eps)
    finally:
        GenConViT.concurrent = True
    torch.cuda.synchronize()
    assert a.shape == (12, 2) and torch.equal(a, b) and torch.equal(a, c)
    # a second current stream: the fork / join must order against whatever stream the caller is on
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        d = g(x, eps=eps)
    s.synchronize()
    assert torch.equal(a, d)


def test_rccl_allgather_through_the_c_abi_world_size_1():
    """gcv_comm_create / gcv_allgather_logits on RCCL with a single rank (the 1-GPU box), directly and through
    genconvit_amd.dist.gather_logits on an "nccl" process group; no 1 -> 8 curve has been measured on hardware."""
    import torch.distributed as tdist
    from genconvit_amd import dist as gdist
    uid = _lib.Comm.unique_id()
    assert len(uid) == 128
    c = _lib.Comm(1, 0, uid, 0)
    t = torch.arange(24, dtype=torch.float32, device="cuda").reshape(2, 6, 2)
    out = c.allgather(t)
    torch.cuda.synchronize()
    assert out.shape == (1, 2, 6, 2) and torch.equal(out[0], t)
    c.close()
    if not tdist.is_initialized():
        import os
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        os.environ.setdefault("MASTER_PORT", "29541")
        tdist.init_process_group("nccl", rank=0, world_size=1, device_id=torch.device("cuda", 0))
        own = True
    else:
        own = False
    try:
        local = torch.randn(10, 2, device="cuda")           # nets = 2, 5 frames
        full = gdist.gather_logits(local, 5, 2)
        assert torch.equal(full, local) and len(gdist._COMMS) == 1
    finally:
        gdist.close_comms()
        if own:
            tdist.destroy_process_group()


def test_in_place_weight_edits_and_oversize_batches(sd_ed):
    """The packed device copy follows in-place edits of the nn.Parameters (the reference's modules would pick them up);
    a batch beyond one handle's 512-frame workspace runs as consecutive chunks (the reference accepts any B)."""
    m = GenConViTED(load_config(), init="empty")
    m.load_state_dict(sd_ed)
    m = m.to("cuda").eval()
    x = synth.make_frames(3, name="edit").cuda()
    a = m(x)
    m.fc2.bias.add_(1.0)                       # in place: bumps the parameter's version counter
    b = m(x)
    assert (b - a - 1.0).abs().max().item() <= 1e-6
    m.fc2.bias.data.sub_(1.0)                  # through .data: invisible to the version check
    m.invalidate()
    assert (m(x) - a).abs().max().item() <= 1e-6
    xb = synth.make_frames(4, name="edit").cuda().repeat(130, 1, 1, 1)      # 520 frames
    big = m(xb)
    assert big.shape == (520, 2) and (big[:4] - big[516:]).abs().max().item() <= 1e-6


# ----------------------------------------------------------------------------- row N4: face crop + INTER_AREA resize
def _boxes_all_regimes(nf, H, W):
    """(frame, top, right, bottom, left) rows covering every branch of cv::resize(INTER_AREA) and the frame borders"""
    return [
        (0, 0, 448, 448, 0),                 # 2x2 whole factor: (a+b+c+d+2)>>2
        (1, 10, 672 + 5, 672 + 10, 5),       # 3x3 whole factor: cvRound(sum / 9)
        (2, 0, 448, 672, 0),                 # 3 (y) x 2 (x)
        (0, 100, 324, 324, 100),             # scale 1: copy
        (1, 33, 47 + 310, 33 + 300, 47),     # general shrink, both axes
        (2, 200, 1000, 200 + 511, 603),      # general shrink, factor > 2 on y
        (3, H - 233, W, H, W - 225),         # barely shrinking, touching the bottom-right corner
        (0, 50, 170, 150, 50),               # both axes grow (100 x 120)
        (1, 5, 405, 155, 5),                 # y grows, x shrinks -> bilinear path for both
        (2, 300, 390, 700, 300),             # x grows, y shrinks
        (3, 7, 8, 8, 7),                     # a single pixel
        (3, 0, 223, 225, 0),                 # 225 x 223: one axis either side of 224
        (nf - 1, 0, W, H, 0),                # the whole frame
    ]


def test_face_crop_resize_is_bit_equal_to_the_inter_area_restatement():
    from oracle import cv_area
    nf, H, W = 4, 720, 1280
    rng = np.random.default_rng(5)
    frames = rng.integers(0, 256, (nf, H, W, 3), dtype=np.uint8)
    yy, xx = np.mgrid[0:H, 0:W]
    frames[3] = np.stack([(yy * 3 + xx) % 256, (xx * 2) % 256, (yy * xx // 97) % 256], -1).astype(np.uint8)   # smooth: ties
    boxes = _boxes_all_regimes(nf, H, W)
    got = _lib.face_crop_resize(torch.as_tensor(frames).cuda(), boxes).cpu().numpy()
    want = cv_area.face_crops(frames, boxes)
    for i, b in enumerate(boxes):
        diff = np.abs(got[i].astype(int) - want[i].astype(int))
        assert diff.max() == 0, f"box {i} {b}: {int((diff > 0).sum())} pixels differ, max {diff.max()}"


def test_face_rec_crops_on_the_device_and_keeps_the_reference_contract():
    from oracle import cv_area
    rng = np.random.default_rng(6)
    frames = rng.integers(0, 256, (3, 360, 640, 3), dtype=np.uint8)
    found = [(0, 20, 300, 280, 40), (0, 100, 500, 200, 400), (2, 0, 640, 360, 0), (2, 5, 50, 50, 5)]   # > len(frames)
    faces, count = pred_func.face_rec(frames, locate=lambda fr: list(found))
    assert count == 3 and isinstance(faces, np.ndarray) and faces.shape == (3, 224, 224, 3) and faces.dtype == np.uint8
    assert np.array_equal(faces, cv_area.face_crops(frames, found[:3]))        # reference :78: at most len(frames) faces
    assert pred_func.face_rec(frames, locate=lambda fr: []) == ([], 0)
    with pytest.raises(_lib.GenConViTHipError):
        _lib.face_crop_resize(torch.as_tensor(frames).cuda(), [(0, 10, 700, 100, 10)])          # right edge outside the frame
    x = pred_func.preprocess_frame(faces)                                        # the next stage of df_face (:139-141)
    assert x.shape == (3, 3, 224, 224) and x.is_cuda


def test_face_crop_resize_random_boxes_are_bit_equal():
    """fuzz: 64 random boxes (sizes from 2 px to the whole frame, any aspect ratio) against the restatement"""
    from oracle import cv_area
    nf, H, W = 3, 480, 640
    rng = np.random.default_rng(11)
    frames = rng.integers(0, 256, (nf, H, W, 3), dtype=np.uint8)
    boxes = []
    for _ in range(64):
        h = int(rng.integers(2, H + 1)) if rng.random() < 0.7 else int(rng.choice([112, 224, 448]))
        w = int(rng.integers(2, W + 1)) if rng.random() < 0.7 else int(rng.choice([112, 224, 448]))
        top, left = int(rng.integers(0, H - h + 1)), int(rng.integers(0, W - w + 1))
        boxes.append((int(rng.integers(0, nf)), top, left + w, top + h, left))
    got = _lib.face_crop_resize(torch.as_tensor(frames).cuda(), boxes).cpu().numpy()
    want = cv_area.face_crops(frames, boxes)
    bad = [(i, boxes[i]) for i in range(len(boxes)) if not np.array_equal(got[i], want[i])]
    assert not bad, f"{len(bad)} boxes differ, first: {bad[0]}"
