"""CPU tests of the oracle (oracle/cpu_ref.py): it must reproduce the committed golden
vectors (made by the reference's own classes, tests/golden/make_golden.py) and agree with
the independent Hugging Face implementation of ConvNeXt-T / Swin-T."""
import os

import numpy as np
import pytest
import torch

from genconvit_amd import spec, synth
from oracle import cpu_ref

torch.set_grad_enabled(False)


def slice64(t):
    f = t.detach().flatten()
    idx = torch.linspace(0, f.numel() - 1, 64).long()
    return f[idx].numpy()


def test_generator_matches_numpy_restatement():
    key = synth._name_key(synth.DEFAULT_SEED, "probe")
    a = synth._splitmix_bits24(key, 12345, 4096).numpy()
    b = synth.splitmix_bits24_numpy(key, 12345, 4096)
    assert np.array_equal(a, b)
    u = synth.uniform01("probe", 1 << 16)
    assert 0.0 <= float(u.min()) and float(u.max()) < 1.0
    assert abs(float(u.mean()) - 0.5) < 0.01
    n = synth.normal("probe", (1 << 16,))
    assert abs(float(n.mean())) < 0.02 and abs(float(n.std()) - 1.0) < 0.02


def test_generator_known_answers():
    # frozen values: the generator must never drift (golden logits depend on it)
    u = synth.uniform01("probe", 4)
    assert u.dtype == torch.float32
    assert [int(v * (1 << 24)) for v in u.tolist()] == \
        synth.splitmix_bits24_numpy(synth._name_key(synth.DEFAULT_SEED, "probe"), 0, 4).tolist()
    x = synth.make_frames(1)
    assert x.shape == (1, 3, 224, 224)
    assert -2.2 < float(x.min()) < -2.0 and 2.5 < float(x.max()) < 2.7


def test_param_counts():
    n_cnx = sum(int(np.prod(s)) for _, s, _ in spec.convnext_tiny_spec(""))
    assert n_cnx == 28_589_128                      # published convnext_tiny count
    n_swin = sum(int(np.prod(s)) for _, s, _ in spec.swin_tiny_spec(""))
    assert n_swin == 28_288_354                     # published swin_tiny count
    ed_ae = sum(int(np.prod(s)) for n, s, _ in spec.ed_spec() if n.startswith(("encoder.", "decoder.")))
    assert ed_ae == 567_123
    vae_enc = sum(int(np.prod(s)) for n, s, k in spec.vae_spec() if n.startswith("encoder.")
                  and k not in ("bn_mean", "bn_var"))
    assert vae_enc == 635_986_432
    vae_dec = sum(int(np.prod(s)) for n, s, _ in spec.vae_spec() if n.startswith("decoder."))
    assert vae_dec == 76_083


def test_ed_matches_reference_golden(golden, sd_ed):
    x = synth.make_frames(4)
    taps = {}
    logits = cpu_ref.ed_forward(sd_ed, x, taps)
    assert np.allclose(logits.numpy(), golden["ed_logits"], rtol=0, atol=2e-6)
    assert np.allclose(slice64(taps["ed_feat"]), golden["ed_feat_slice"], rtol=0, atol=2e-5)
    enc = cpu_ref.ed_encoder(sd_ed, x[:2])
    assert np.allclose(slice64(enc), golden["ed_enc_slice"], rtol=1e-6, atol=1e-6)
    assert np.allclose(slice64(cpu_ref.ed_decoder(sd_ed, enc)), golden["ed_dec_slice"], rtol=1e-6, atol=1e-6)


def test_vae_matches_reference_golden(golden, sd_vae):
    x = synth.make_frames(4)
    eps = torch.from_numpy(golden["vae_eps"])
    logits, recon, kl = cpu_ref.vae_forward(sd_vae, x, eps, want_kl=True)
    assert np.allclose(logits.numpy(), golden["vae_logits"], rtol=0, atol=2e-6)
    assert np.allclose(slice64(recon), golden["vae_recon_slice"], rtol=1e-6, atol=1e-6)
    assert abs(float(kl) - float(golden["vae_kl"])) <= 1e-5 * abs(float(golden["vae_kl"]))
    assert np.allclose(cpu_ref.mse_per_frame(recon, x).numpy(), golden["vae_mse"], rtol=1e-6)
    # the reference's redundant 3x mu + var evaluation gives the same z
    z_a, _ = cpu_ref.vae_encoder(sd_vae, x[:1], eps[:1], as_written=True)
    z_b, _ = cpu_ref.vae_encoder(sd_vae, x[:1], eps[:1], as_written=False)
    assert torch.equal(z_a, z_b)


def test_reference_16bit_runs_are_recorded_beside_the_fp32_golden(golden):
    """tests/golden/make_golden.py also runs the reference's own classes after .half() / .bfloat16() (its --fp16 path,
    model/genconvit.py:24-25): the committed deltas are the yardstick of the 16-bit GPU tests."""
    want = {("ed", "half"): 9.3e-4, ("vae", "half"): 6.8e-4, ("ed", "bf16"): 7.8e-3, ("vae", "bf16"): 5.6e-3}
    for (net, d), v in want.items():
        got = np.abs(golden[f"{net}_logits_{d}"] - golden[f"{net}_logits"]).max()
        assert abs(got - v) <= 0.02 * v + 1e-5, (net, d, got)


def test_vote_matches_reference_golden(golden):
    logits = torch.from_numpy(golden["genconvit_logits"])
    y, val = cpu_ref.vote(logits)
    assert y == int(golden["vote_idx"])
    assert abs(val - float(golden["vote_val"])) < 1e-7
    assert {0: "REAL", 1: "FAKE"}[y ^ 1] == str(golden["vote_label"])


def test_hybrid_embed_probe_dims(golden):
    # model/model_embedder.py:16-37 with a (1,1000)-logit embedder: grid (1,1000), proj 1000->768
    assert golden["hybrid_grid"].tolist() == [1, 1000]
    assert golden["hybrid_proj_shape"].tolist() == [768, 1000, 1, 1]


def _hf_convnext(sd):
    from transformers import ConvNextConfig, ConvNextForImageClassification
    m = ConvNextForImageClassification(ConvNextConfig(num_labels=1000, layer_norm_eps=1e-6)).eval()
    new = {}
    new["convnext.embeddings.patch_embeddings.weight"] = sd["stem.0.weight"]
    new["convnext.embeddings.patch_embeddings.bias"] = sd["stem.0.bias"]
    new["convnext.embeddings.layernorm.weight"] = sd["stem.1.weight"]
    new["convnext.embeddings.layernorm.bias"] = sd["stem.1.bias"]
    for i, depth in enumerate(spec.CONVNEXT_DEPTHS):
        if i > 0:
            for a in (0, 1):
                for wb in ("weight", "bias"):
                    new[f"convnext.encoder.stages.{i}.downsampling_layer.{a}.{wb}"] = \
                        sd[f"stages.{i}.downsample.{a}.{wb}"]
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


@pytest.mark.parametrize("res", [224, 112])
def test_convnext_restatement_vs_huggingface(res):
    """ConvNeXt-T lives in absent timm==0.6.5 (parity unpinned by the reference); the
    restatement is cross-checked against an independent implementation of the same
    published architecture, at both resolutions the path uses (224 and the VAE's 112)."""
    sd = synth.make_state_dict(spec.convnext_tiny_spec(""), tag="hfcheck/")
    m = _hf_convnext(sd)
    x = synth.make_frames(2)
    if res != 224:
        x = torch.nn.functional.avg_pool2d(x, 2)
    ours = cpu_ref.convnext_tiny(sd, "", x)
    theirs = m(pixel_values=x).logits
    assert float((ours - theirs).abs().max()) < 2e-5
    assert float(ours.abs().max()) > 0.5           # non-degenerate


def _hf_swin(sd):
    from transformers import SwinConfig, SwinForImageClassification
    m = SwinForImageClassification(SwinConfig(num_labels=1000)).eval()
    hs = m.state_dict()
    new = {}
    new["swin.embeddings.patch_embeddings.projection.weight"] = sd["patch_embed.proj.weight"]
    new["swin.embeddings.patch_embeddings.projection.bias"] = sd["patch_embed.proj.bias"]
    new["swin.embeddings.norm.weight"] = sd["patch_embed.norm.weight"]
    new["swin.embeddings.norm.bias"] = sd["patch_embed.norm.bias"]
    for i, (dim, depth) in enumerate(zip(spec.SWIN_DIMS, spec.SWIN_DEPTHS)):
        for j in range(depth):
            s, d = f"layers.{i}.blocks.{j}.", f"swin.encoder.layers.{i}.blocks.{j}."
            qkv_w, qkv_b = sd[s + "attn.qkv.weight"], sd[s + "attn.qkv.bias"]
            for n, nm in enumerate(("q_proj", "k_proj", "v_proj")):
                new[d + f"attention.{nm}.weight"] = qkv_w[n * dim:(n + 1) * dim]
                new[d + f"attention.{nm}.bias"] = qkv_b[n * dim:(n + 1) * dim]
            new[d + "attention.o_proj.weight"] = sd[s + "attn.proj.weight"]
            new[d + "attention.o_proj.bias"] = sd[s + "attn.proj.bias"]
            new[d + "attention.relative_position_bias.relative_position_bias_table"] = \
                sd[s + "attn.relative_position_bias_table"]
            for a, b in (("norm1", "layernorm_before"), ("norm2", "layernorm_after"),
                         ("mlp.fc1", "mlp.fc1"), ("mlp.fc2", "mlp.fc2")):
                for wb in ("weight", "bias"):
                    new[d + f"{b}.{wb}"] = sd[s + f"{a}.{wb}"]
        if i < 3:
            s, d = f"layers.{i}.downsample.", f"swin.encoder.layers.{i}.downsample."
            new[d + "reduction.weight"] = sd[s + "reduction.weight"]
            new[d + "norm.weight"] = sd[s + "norm.weight"]
            new[d + "norm.bias"] = sd[s + "norm.bias"]
    new["swin.layernorm.weight"] = sd["norm.weight"]
    new["swin.layernorm.bias"] = sd["norm.bias"]
    new["classifier.weight"] = sd["head.weight"]
    new["classifier.bias"] = sd["head.bias"]
    extra = {k: v for k, v in hs.items() if k not in new}      # index buffers, if registered
    missing = [k for k in extra if "relative_position_index" not in k and "mask" not in k]
    assert not missing, missing
    new.update(extra)
    m.load_state_dict(new, strict=True)
    return m


def test_swin_restatement_vs_huggingface():
    sd = synth.make_state_dict(spec.swin_tiny_spec(""), tag="hfcheck/")
    m = _hf_swin(sd)
    x = synth.make_frames(2)
    ours = cpu_ref.swin_tiny(sd, "", x)
    theirs = m(pixel_values=x).logits
    assert float((ours - theirs).abs().max()) < 5e-5
    assert float(ours.abs().max()) > 0.5


def test_oracle_architecture_constants_are_its_own_and_agree_with_the_product():
    """oracle/cpu_ref.py must not import its architecture table from the product; the two copies must agree."""
    import re
    src = open(cpu_ref.__file__).read()
    assert not re.search(r"^\s*from genconvit_amd|^\s*import genconvit_amd", src, re.M)
    assert tuple(cpu_ref.CONVNEXT_DEPTHS) == tuple(spec.CONVNEXT_DEPTHS) and tuple(cpu_ref.CONVNEXT_DIMS) == tuple(spec.CONVNEXT_DIMS)
    assert tuple(cpu_ref.SWIN_DEPTHS) == tuple(spec.SWIN_DEPTHS) and tuple(cpu_ref.SWIN_DIMS) == tuple(spec.SWIN_DIMS)
    assert tuple(cpu_ref.SWIN_HEADS) == tuple(spec.SWIN_HEADS)


def test_committed_huggingface_fixture_is_what_the_script_produces(tmp_path):
    """tests/golden/hf_backbones.npz must be reproducible from tests/golden/make_hf_golden.py.  The float32 reductions of
    the CPU kernels run in an order that depends on the host's vector ISA and thread count, so a rerun on another host
    (or with another torch.set_num_threads) moves the logits by a few ulps (<= 2e-6 seen at |logit| <= 4); the bound below
    is ten times that, under the 5e-5 / 1e-4 the script itself allows between Hugging Face and the oracle, and orders of
    magnitude under what any change of weights, frames or architecture produces."""
    import importlib.util
    import numpy as np
    here = os.path.dirname(os.path.abspath(__file__))
    s = importlib.util.spec_from_file_location("make_hf_golden", os.path.join(here, "golden", "make_hf_golden.py"))
    mod = importlib.util.module_from_spec(s)
    s.loader.exec_module(mod)
    out = str(tmp_path / "hf.npz")
    mod.main(out)
    new, old = dict(np.load(out)), dict(np.load(os.path.join(here, "golden", "hf_backbones.npz")))
    assert set(new) == set(old)
    for k in old:
        assert new[k].shape == old[k].shape and new[k].dtype == old[k].dtype, k
        assert np.abs(new[k] - old[k]).max() <= 2e-5, (k, float(np.abs(new[k] - old[k]).max()))


# ----------------------------------------------------------------------------- row N4: cv2.INTER_AREA restatement
# (parity unpinned against OpenCV itself — cv2 is not installed and the reference holds no fixture; these pin the
# restatement to the definition of area resampling and to an independent implementation where one exists)
def _sep(Wy, img, Wx):
    """(Wy . img . Wx^T) per channel, in float64"""
    return np.einsum("yh,hxc->yxc", Wy, np.einsum("hwc,xw->hxc", img.astype(np.float64), Wx))


def _area_weights(s, d):
    scale = s / d
    W = np.zeros((d, s))
    for dx in range(d):
        a, b = dx * scale, min((dx + 1) * scale, s)
        for sx in range(int(np.floor(a)), min(int(np.ceil(b)), s)):
            W[dx, sx] = max(0.0, min(b, sx + 1) - max(a, sx))
        W[dx] /= W[dx].sum()
    return W


@pytest.mark.parametrize("h,w", [(300, 310), (225, 500), (233, 224), (511, 397)])
def test_cv_area_general_shrink_is_the_rounded_exact_area_mean(h, w):
    from oracle import cv_area
    src = np.random.default_rng(h * 1000 + w).integers(0, 256, (h, w, 3), dtype=np.uint8)
    out = cv_area.resize_area_u8(src)
    exact = _sep(_area_weights(h, 224), src, _area_weights(w, 224))
    assert np.abs(out - exact).max() <= 0.5 + 1e-3          # fp32 running sums: a tie may round either way


@pytest.mark.parametrize("fy,fx", [(2, 2), (3, 3), (2, 3), (4, 1), (1, 1)])
def test_cv_area_whole_factors_are_block_means_and_match_pillow_box(fy, fx):
    from oracle import cv_area
    src = np.random.default_rng(fy * 10 + fx).integers(0, 256, (224 * fy, 224 * fx, 3), dtype=np.uint8)
    out = cv_area.resize_area_u8(src)
    mean = src.reshape(224, fy, 224, fx, 3).astype(np.float64).mean(axis=(1, 3))
    assert np.abs(out - mean).max() <= 0.5
    if fy == fx == 1:
        assert np.array_equal(out, src)
    PIL = pytest.importorskip("PIL.Image")                  # an independent area-averaging resampler
    box = np.asarray(PIL.fromarray(src).resize((224, 224), PIL.BOX))
    assert np.abs(out.astype(int) - box.astype(int)).max() <= 1


@pytest.mark.parametrize("h,w", [(100, 120), (150, 400), (400, 90), (1, 1), (223, 225)])
def test_cv_area_growing_dimension_is_area_mode_bilinear(h, w):
    """as soon as a dimension grows OpenCV interpolates between the two source pixels a destination cell overlaps, with
    the overlap fractions as weights: the integer H / V passes against the same weights applied in floating point"""
    from oracle import cv_area
    src = np.random.default_rng(h * 7 + w).integers(0, 256, (h, w, 3), dtype=np.uint8)
    out = cv_area.resize_area_u8(src)

    def weights(s, d):                                      # the fp32 overlap fractions, before the 11-bit rounding
        ofs, coef, _ = cv_area._linear_tab(s, d, 1.0 / (d / s), d / s)
        W = np.zeros((d, s))
        for i in range(d):
            W[i, ofs[i]] += coef[i][0] / cv_area.COEF_SCALE
            if coef[i][1]:
                W[i, ofs[i] + 1] += coef[i][1] / cv_area.COEF_SCALE
        assert np.allclose(W.sum(1), 1.0, atol=1e-3) and (W >= 0).all()
        return W
    want = _sep(weights(h, 224), src, weights(w, 224))
    assert np.abs(out - want).max() <= 1.0                  # 11-bit coefficients, truncating shifts
    flat = cv_area.resize_area_u8(np.full((h, w, 3), 137, dtype=np.uint8))
    assert np.all(flat == 137)


def test_face_crop_needs_the_gpu_and_never_falls_back():
    from genconvit_amd import _lib
    from genconvit_amd.model import pred_func
    if torch.cuda.is_available():
        pytest.skip("CPU-only check")
    frames = np.zeros((2, 64, 64, 3), dtype=np.uint8)
    with pytest.raises(_lib.GenConViTHipError):
        pred_func.face_rec(frames, locate=lambda fr: [(0, 4, 40, 40, 4)])
    assert pred_func.face_rec(frames, locate=lambda fr: []) == ([], 0)       # reference :92
