"""Stage-by-stage 16-bit (and fp32) evidence at the benchmarked batch sizes: every tap of the ED and VAE forwards
(include/genconvit_hip.h, gcv_tap_set) against the oracle's same-dtype restatement (oracle/cpu_ref.py, storage_dtype),
element by element.  The (B, 2) logits average a localized kernel error away (a 32-token tile that skips a whole block
moves them by about the fp16 logit bound); at the activations the same error is two orders of magnitude above the
bounds below (tests/test_host_cpu.py, test_tap_check_catches_a_skipped_tile).

Bounds: taputil.BOUNDS, max |got - want| / rms(want) per tap kind, about 3x what was measured on the MI355X.
"""
import pytest
import torch

from genconvit_amd import _lib, synth
from genconvit_amd.model.config import load_config
from genconvit_amd.model.genconvit_vae import GenConViTVAE
from oracle import cpu_ref
from tests import taputil

pytestmark = pytest.mark.gpu
torch.set_grad_enabled(False)

_HANDLES = {}


def _sd(net):
    from tests.conftest import synthetic_sd
    return synthetic_sd(net)


def _handle(net, dtype, max_batch=128):
    """One cached handle per (network, dtype); the VAE without encoder.var (the taps never need the KL)."""
    key = (net, dtype, max_batch)
    if key not in _HANDLES:
        h = _lib.Handle(0, dtype, max_batch)
        if net == "ed":
            h.load_ed(_sd("ed"))
        else:
            h.load_vae(_sd("vae"), with_var=False)
        _HANDLES[key] = h
    return _HANDLES[key]


def _oracle(net, dtype, x, eps, merged):
    taps = {}
    with cpu_ref.storage_dtype(dtype):
        if net == "ed":
            cpu_ref.ed_forward(_sd("ed"), x, taps)
        else:
            cpu_ref.vae_forward(_sd("vae"), x, eps, taps=taps, merged=merged)
    return taps


def run_case(dtype, B, handles, forward, merged, name):
    """Taps on every handle of ``handles`` (net -> Handle), one ``forward(x, eps)``, then each network against the oracle
    (``merged``: the VAE ran its two backbone passes as one launch).  Returns the rows of taputil.compare per network."""
    x = synth.make_frames(B, name=name)
    eps = synth.make_eps(B, name=name)
    bufs = {net: taputil.set_taps(h, net, B, dtype) for net, h in handles.items()}
    try:
        forward(x.to("cuda", dtype), eps.cuda())
        torch.cuda.synchronize()
        written = {net: {n: handles[net].tap_written(n) for n in bufs[net]} for net in handles}
    finally:
        for h in handles.values():
            h.clear_taps()
    out = {}
    for net in handles:
        want = _oracle(net, dtype, x, eps, merged)
        out[net] = taputil.compare(bufs[net], want, taputil.layout(net, B), taputil.BOUNDS[dtype], written[net])
        del want
    return out


def _check(results, title):
    msgs = []
    for net, rows in results.items():
        print("\n" + taputil.report(rows, f"{title}: {net}"))
        msgs += [r["where"] for r in taputil.failures(rows)]
    assert not msgs, f"{title}: {len(msgs)} tap(s) out of bounds; first: {msgs[0]}"


def _ensemble(dtype):
    he, hv = _handle("ed", dtype), _handle("vae", dtype)
    return {"ed": he, "vae": hv}, lambda x, eps: _lib.genconvit_forward(he, hv, x, eps)


# ----------------------------------------------------------------------------- configurations
def test_taps_ed_batch32_fp32():
    """BASELINE configs[1]: ED, B = 32, fp32, against the fp32 oracle."""
    h = _handle("ed", torch.float32, 32)
    _check(run_case(torch.float32, 32, {"ed": h}, lambda x, eps: h.ed_forward(x), False, "cfg2"), "ED fp32 B=32")


@pytest.mark.parametrize("split", [True, False])
def test_taps_vae_batch32_bf16_both_schedules(split, monkeypatch):
    """BASELINE configs[2]: VAE, B = 32, bf16, under both gcv_vae_forward schedules (backbone(x) on the side stream, or
    one merged two-segment pass): the taps of the side-stream pass are copied on that stream."""
    monkeypatch.setenv("GCV_VAE_SPLIT", "1" if split else "0")
    h = _lib.Handle(0, torch.bfloat16, 32)      # the switch is read when the handle is created
    h.load_vae(_sd("vae"), with_var=False)
    try:
        res = run_case(torch.bfloat16, 32, {"vae": h}, lambda x, eps: h.vae_forward(x, eps, want_recon=False), not split,
                       "cfg3")
    finally:
        h.close()
    _check(res, f"VAE bf16 B=32 split={split}")


def test_taps_genconvit_batch128_fp16(monkeypatch):
    """BASELINE configs[3]: both networks through gcv_genconvit_forward, B = 128, fp16 (LDS-resident C = 96 MLP with its
    LayerNorm-patchify epilogue, matrix-pipe depthwise kernel, multi-pass persistent C = 192 / 384 launches)."""
    monkeypatch.delenv("GCV_VAE_SPLIT", raising=False)
    handles, fwd = _ensemble(torch.float16)
    _check(run_case(torch.float16, 128, handles, fwd, True, "cfg4"), "genconvit fp16 B=128")


@pytest.mark.parametrize("B", [4, 33, 67])
@pytest.mark.parametrize("dtype", [torch.float16, torch.bfloat16], ids=["f16", "bf16"])
def test_taps_genconvit_odd_and_small_batches(dtype, B, monkeypatch):
    """B = 33 / 67: tiles straddle the segment boundaries of the two-segment token streams; B = 4: the small-M kernels."""
    monkeypatch.delenv("GCV_VAE_SPLIT", raising=False)
    handles, fwd = _ensemble(dtype)
    _check(run_case(dtype, B, handles, fwd, True, "odd"), f"genconvit {dtype} B={B}")


# ----------------------------------------------------------------------------- the hook's contract
def test_tap_errors_and_removal():
    h = _handle("ed", torch.float16)
    with pytest.raises(_lib.GenConViTHipError, match="unknown tap"):
        h.set_tap("ed.bb.s0.b3", torch.empty(8, dtype=torch.float16, device="cuda"))
    with pytest.raises(_lib.GenConViTHipError, match="no tap"):
        h.tap_written("ed.e1")
    x = synth.make_frames(2).to("cuda", torch.float16)
    ref = h.ed_forward(x)
    # a buffer of the wrong size fails the forward with a message that names the tap
    h.set_tap("ed.e1", torch.empty(2 * 112 * 112 * 16 - 1, dtype=torch.float16, device="cuda"))
    with pytest.raises(_lib.GenConViTHipError, match="tap 'ed.e1'"):
        h.ed_forward(x)
    torch.cuda.synchronize()
    # right size: written; removed: no longer copied; taps change nothing else
    buf = torch.full((2 * 112 * 112 * 16,), float("nan"), dtype=torch.float16, device="cuda")
    h.set_tap("ed.e1", buf)
    assert torch.equal(h.ed_forward(x), ref)
    torch.cuda.synchronize()
    assert h.tap_written("ed.e1") and not torch.isnan(buf).any()
    h.set_tap("ed.e1", None)
    buf.fill_(float("nan"))
    assert torch.equal(h.ed_forward(x), ref)
    torch.cuda.synchronize()
    assert torch.isnan(buf).all()
    h.clear_taps()


# ----------------------------------------------------------------------------- Encoder.kl beyond one handle
def test_vae_kl_over_512_frames_is_the_batch_mean():
    """B > 512 runs as chunks of 512; Encoder.kl is the mean over the whole batch (model/genconvit_vae.py:58), so the
    chunks' KLs are weighted by their frame counts.  512 copies of one frame and 8 of another have different chunk KLs."""
    sd = _sd("vae")
    x2 = synth.make_frames(2, name="kl")
    e2 = synth.make_eps(2, name="kl")
    x = torch.cat([x2[0:1].expand(512, -1, -1, -1), x2[1:2].expand(8, -1, -1, -1)]).contiguous()
    eps = torch.cat([e2[0:1].expand(512, -1), e2[1:2].expand(8, -1)]).contiguous()
    m = GenConViTVAE(load_config(), init="empty")
    m.load_state_dict(sd)
    m = m.to("cuda").eval()
    m(x.cuda(), eps=eps.cuda(), want_recon=False, want_kl=True)
    got = float(m.kl)
    kl_a = cpu_ref.vae_encoder(sd, x2[0:1], e2[0:1], want_kl=True)[1].item()
    kl_b = cpu_ref.vae_encoder(sd, x2[1:2], e2[1:2], want_kl=True)[1].item()
    want = (512 * kl_a + 8 * kl_b) / 520
    print(f"\nVAE fp32 B=520: kl {got:.6g}, batch mean {want:.6g} (frame a {kl_a:.6g}, frame b {kl_b:.6g})")
    assert abs(kl_a - kl_b) > 1e-2 * abs(want), "the two chunks must differ for this test to mean anything"
    assert abs(got - want) <= 1e-4 * abs(want)
    del m
    _release()


def _release():
    torch.cuda.synchronize()
    torch.cuda.empty_cache()
