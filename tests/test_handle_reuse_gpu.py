"""No memory between calls, on the MI355X: a handle with a past gives the bits of a handle without one.

The arena is a stack that every forward lays out again; `cur`, `in_ensemble`, `after_chain`, `Arena::overflow`, the tap masks
and `prof.enabled` are members one call sets and the next one reads; split-K partials and bias-initialised accumulators
sit in workspace an earlier, larger call has written.  Per dtype three probes are recorded ONCE, each as the very first
call of brand-new handles (streamutil.fresh):
    ed_forward at B = 2;  vae_forward at B = 2 with recon, mse and kl;  genconvit_forward at B = 2.
One long-lived pair of handles then goes through the steps below; after each step the probes run again and every tensor
must be torch.equal to the recorded one.  The VAE handles are created with GCV_VAE_SPLIT unset, the default: the split
schedule when called alone, the merged one inside the ensemble — the switch `in_ensemble` that an ensemble call must reset.
The long-lived VAE handle is reserve(16), the ED handle the default 32, so that one ensemble batch is within the ED
handle's max_batch and above the VAE's (the refusal after the ED network was enqueued)."""
import pytest
import torch

from genconvit_amd import _lib, synth
from tests import streamutil as su

pytestmark = pytest.mark.gpu
torch.set_grad_enabled(False)

F16, F32 = torch.float16, torch.float32
DTYPES = [pytest.param(F16, id="fp16"), pytest.param(F32, id="fp32")]
VAE_MAX = 16
_W = {}


def ensemble(m_ed, m_vae):
    from genconvit_amd.model.genconvit import GenConViT
    return GenConViT.from_modules(m_ed, m_vae, net="genconvit")


class World:
    def __init__(self, dtype, mp):
        self.dtype = dtype
        dev = lambda t: t.to("cuda").to(dtype).contiguous()
        self.x2, self.eps2 = dev(synth.make_frames(2, name="reuse.probe")), synth.make_eps(2, name="reuse.probe").cuda()
        self.x4, self.eps4 = dev(synth.make_frames(4, name="reuse.b4")), synth.make_eps(4, name="reuse.b4").cuda()
        self.base_ed, self.base_vae = su.base_model("ed", dtype), su.base_model("vae", dtype)
        torch.cuda.synchronize()
        # the ensemble probe: the first call of two brand-new handles, which are then dropped
        e, v = self.new_ed(), self.new_vae(mp, VAE_MAX)
        self.want = {"ens": self.run("ens", e, v)}
        del e, v
        # the long-lived pair; its first calls are the ED-alone and the VAE-alone probe
        self.ed, self.vae = self.new_ed(), self.new_vae(mp, VAE_MAX)
        self.want["ed"] = self.run("ed", self.ed, None)
        self.want["vae"] = self.run("vae", None, self.vae)

    def new_ed(self, max_batch=None):
        return su.fresh(self.base_ed, max_batch=max_batch)

    def new_vae(self, mp, max_batch=None, keep_kl_weights=True):
        return su.fresh(self.base_vae, max_batch=max_batch, split=None, monkeypatch=mp, keep_kl_weights=keep_kl_weights, batch=2)

    def run(self, which, e, v):
        """The probe `which` on the modules (e, v): its tensors, cloned, everything synchronised."""
        if which == "ed":
            outs = [e(self.x2)]
        elif which == "vae":
            logits, recon = v(self.x2, eps=self.eps2, want_recon=True, want_mse=True, want_kl=v.keep_kl_weights)
            outs = [logits, recon, v.mse] + ([v.kl] if v.keep_kl_weights else [])
        else:
            outs = [ensemble(e, v)(self.x2, eps=self.eps2)]
        outs = [o.clone() for o in outs]
        torch.cuda.synchronize()
        return outs

    def check(self, after, which=("vae", "ed", "ens"), e=None, v=None, want=None):
        e, v = e or self.ed, v or self.vae
        for w in which:
            got, ref = self.run(w, e, v), (want or self.want)[w]
            assert len(got) == len(ref)
            for i, (a, b) in enumerate(zip(got, ref)):
                assert a.shape == b.shape and bool(torch.isfinite(a.float()).all())
                assert torch.equal(a, b), (f"{self.dtype}: after {after}, tensor #{i} of the {w} probe differs from the one "
                                           f"recorded on brand-new handles: max |diff| {(a.float() - b.float()).abs().max().item():.3e}, "
                                           f"{int((a != b).sum())} of {a.numel()} elements")


def world(dtype, mp) -> World:
    if dtype not in _W:
        _W[dtype] = World(dtype, mp)
    return _W[dtype]


def vae_all(w, x, eps, **kw):
    kw = kw or dict(want_recon=True, want_mse=True, want_kl=True)
    logits, recon = w.vae(x, eps=eps, **kw)
    return [logits, recon, w.vae.mse, w.vae.kl]


def finite(*ts):
    for t in su.flat(list(ts)):
        assert bool(torch.isfinite(t.float()).all())


@pytest.mark.parametrize("dtype", DTYPES)
def test_the_three_probes_agree(dtype, monkeypatch):
    """The ensemble's rows are the two networks' own logits (what test_parity_gpu.py holds at fp32, B = 6)."""
    w = world(dtype, monkeypatch)
    assert torch.equal(w.want["ens"][0][:2], w.want["ed"][0]) and torch.equal(w.want["ens"][0][2:], w.want["vae"][0])
    w.check("nothing")


@pytest.mark.parametrize("dtype", DTYPES)
def test_after_a_hot_batch_of_9(dtype, monkeypatch):
    """Every arena byte the probes use then holds foreign data: all-255 and all-0 frames through gcv_preprocess, interleaved
    (the extremes of the input range, +-2.6 after normalisation), eps x 4.  Finite throughout."""
    w = world(dtype, monkeypatch)
    u8 = torch.zeros((9, 224, 224, 3), dtype=torch.uint8, device="cuda")
    u8[0::2] = 255
    x = _lib.preprocess(u8, dtype)
    eps = synth.make_eps(9, name="reuse.hot").cuda() * 4.0
    finite(x, eps, w.ed(x), vae_all(w, x, eps), ensemble(w.ed, w.vae)(x, eps=eps))
    torch.cuda.synchronize()
    w.check("a forward at B = 9 on hot inputs")


@pytest.mark.parametrize("dtype", DTYPES)
def test_after_a_batch_of_1(dtype, monkeypatch):
    w = world(dtype, monkeypatch)
    finite(w.ed(w.x4[:1]), vae_all(w, w.x4[:1], w.eps4[:1]), ensemble(w.ed, w.vae)(w.x4[:1], eps=w.eps4[:1]))
    w.check("a forward at B = 1")


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("layer", ["s3", "s2"])
def test_after_explain_at_batch_4(layer, dtype, monkeypatch):
    """explain keeps buffers the plain forward overwrites (and at "s2" the inputs of stage 3): the probe then runs through
    the plain forward over that layout."""
    w = world(dtype, monkeypatch)
    finite(w.ed.explain(w.x4, layer=layer), w.vae.explain(w.x4, eps=w.eps4, layer=layer),
           ensemble(w.ed, w.vae).explain(w.x4, eps=w.eps4, layer=layer))
    w.check(f"explain at {layer}, B = 4")


@pytest.mark.parametrize("dtype", DTYPES)
def test_after_vae_forward_without_and_with_its_optional_outputs(dtype, monkeypatch):
    w = world(dtype, monkeypatch)
    finite(vae_all(w, w.x4, w.eps4, want_recon=False, want_mse=False, want_kl=False)[0])
    w.check("vae_forward without recon, mse and kl", which=("vae",))
    finite(vae_all(w, w.x4, w.eps4))
    w.check("vae_forward with recon, mse and kl")


@pytest.mark.parametrize("dtype", DTYPES)
def test_after_taps_were_set_and_cleared(dtype, monkeypatch):
    from tests import taputil
    w = world(dtype, monkeypatch)
    keep = []
    for net, m, names in (("ed", w.ed, ("ed.e5", "ed.feat", "ed.bb.pool")), ("vae", w.vae, ("vae.z", "vae.feat", "vae.bb.pool"))):
        h, lay = m._get_handle(2), taputil.layout(net, 2)
        for name in names:
            n = sum(s[1] * s[2] * s[3] for s in lay[name][1])
            keep.append(torch.zeros((n,), dtype=F32 if lay[name][0] else dtype, device="cuda"))
            h.set_tap(name, keep[-1])
    try:
        finite(w.ed(w.x4[:2]), vae_all(w, w.x4[:2], w.eps4[:2]), ensemble(w.ed, w.vae)(w.x4[:2], eps=w.eps4[:2]))
        torch.cuda.synchronize()
        assert all(bool(t.float().abs().sum() > 0) for t in keep), "a tap buffer was never written"
    finally:
        w.ed._get_handle(2).clear_taps()
        w.vae._get_handle(2).clear_taps()
    w.check("three taps per network, one forward, clear_taps")


@pytest.mark.parametrize("dtype", DTYPES)
def test_after_a_profiled_forward(dtype, monkeypatch):
    """The profiled step itself is not compared (it runs the merged schedule on one stream); prof.enabled must be off again."""
    w = world(dtype, monkeypatch)
    he, hv = w.ed._get_handle(2), w.vae._get_handle(2)
    try:
        he.profile_enable(True)
        hv.profile_enable(True)
        finite(w.ed(w.x4), vae_all(w, w.x4, w.eps4))
        assert len(he.profile_report()) > 0 and len(hv.profile_report()) > 0
    finally:
        he.profile_enable(False)
        hv.profile_enable(False)
    w.check("profile_enable(True), a forward, profile_report(), profile_enable(False)")


@pytest.mark.parametrize("dtype", DTYPES)
def test_after_convnext_forward_at_64_and_112(dtype, monkeypatch):
    from tests import kutil
    w = world(dtype, monkeypatch)
    for res in (64, 112):
        x = kutil.frames_at(res, 3).to("cuda").to(dtype)
        finite(w.ed.backbone_forward(x), w.vae.backbone_forward(x))
    w.check("convnext_forward at res 64 and 112")


def _refused(rc, what):
    err = _lib.last_error()
    assert rc != 0 and err, f"{what} was not refused (rc = {rc}, error text {err!r})"
    torch.cuda.synchronize()
    return err


@pytest.mark.parametrize("dtype", DTYPES)
def test_after_calls_the_c_abi_refuses(dtype, monkeypatch):
    w = world(dtype, monkeypatch)
    lib = _lib.load()
    he, hv = w.ed._get_handle(2), w.vae._get_handle(2)
    stream = torch.cuda.current_stream().cuda_stream
    # the ensemble with a batch within the ED handle's max_batch and above the VAE's: the VAE refuses, the ED network is
    # enqueued all the same, and in_ensemble / after_chain must be reset on that way out
    assert hv.max_batch < he.max_batch, "this step needs the ED handle's max_batch above the VAE handle's (run it before the regrowth step)"
    nb = hv.max_batch + 1
    x = w.x4.repeat((nb + 3) // 4, 1, 1, 1)[:nb].contiguous()
    eps = w.eps4.repeat((nb + 3) // 4, 1)[:nb].contiguous()
    out = torch.zeros((2 * nb, 2), device="cuda")
    err = _refused(lib.gcv_genconvit_forward(he._h, hv._h, x.data_ptr(), eps.data_ptr(), nb, out.data_ptr(), stream),
                   f"gcv_genconvit_forward at batch {nb} on a VAE handle of max_batch {hv.max_batch}")
    assert "max_batch" in err
    w.check("a gcv_genconvit_forward the VAE handle refused for its batch", which=("vae", "ed", "ens"))
    # gcv_ed_explain_at with a layer that does not exist
    logits, cam = torch.zeros((2, 2), device="cuda"), torch.zeros((2, 2 * 196), device="cuda")
    _refused(lib.gcv_ed_explain_at(he._h, w.x2.data_ptr(), 2, None, 5, logits.data_ptr(), cam.data_ptr(), None, stream),
             "gcv_ed_explain_at with layer 5")
    w.check("a gcv_ed_explain_at refused for its layer", which=("ed", "ens"))
    # gcv_vae_forward with kl on a handle loaded with_var=False: its own probe (no kl), recorded as its first call
    v = w.new_vae(monkeypatch, VAE_MAX, keep_kl_weights=False)
    first = w.run("vae", None, v)
    for a, b in zip(first, w.want["vae"]):
        assert torch.equal(a, b), "a handle without encoder.var gives other logits / recon / mse than one with it"
    kl = torch.zeros((1,), device="cuda")
    err = _refused(lib.gcv_vae_forward(v._get_handle(2)._h, w.x2.data_ptr(), w.eps2.data_ptr(), 2, logits.data_ptr(), None,
                                       None, kl.data_ptr(), stream), "gcv_vae_forward with kl, encoder.var not loaded")
    assert "encoder.var" in err
    w.check("a gcv_vae_forward refused for kl without encoder.var", which=("vae",), v=v, want={"vae": first})


@pytest.mark.parametrize("dtype", DTYPES)
def test_alone_after_an_ensemble_call(dtype, monkeypatch):
    w = world(dtype, monkeypatch)
    finite(ensemble(w.ed, w.vae)(w.x4, eps=w.eps4))
    w.check("an ensemble call", which=("vae", "ed"))


@pytest.mark.parametrize("dtype", DTYPES)
def test_max_batch_does_not_change_the_bits(dtype, monkeypatch):
    """The arena's size moves every buffer; the kernels and their grids follow the batch, not max_batch."""
    w = world(dtype, monkeypatch)
    for mb in (2, 512):
        e = w.new_ed(mb)
        w.check(f"nothing, on a brand-new ED handle reserve({mb})", which=("ed",), e=e)
        assert e._get_handle(2).max_batch == mb
        del e
    for mb in (2, None):
        v = w.new_vae(monkeypatch, mb)
        w.check(f"nothing, on a brand-new VAE handle reserve({mb or 'default'})", which=("vae",), v=v)
        assert v._get_handle(2).max_batch == (mb or 32)
        del v


@pytest.mark.parametrize("dtype", DTYPES)
def test_after_the_handles_regrew(dtype, monkeypatch):
    """_get_handle: B = 3 on the old handles, then B = 40 makes new ones of max_batch 64 (and packs the weights again)."""
    w = world(dtype, monkeypatch)
    monkeypatch.delenv("GCV_VAE_SPLIT", raising=False)
    x40, eps40 = w.x4.repeat(10, 1, 1, 1), w.eps4.repeat(10, 1)
    for x, eps in ((w.x4[:3], w.eps4[:3]), (x40, eps40)):
        finite(w.ed(x), vae_all(w, x, eps), ensemble(w.ed, w.vae)(x, eps=eps))
    assert w.ed._get_handle(2).max_batch == 64 and w.vae._get_handle(2).max_batch == 64
    w.check("B = 3, then B = 40 on regrown handles")
