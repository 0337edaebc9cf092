"""Stream ordering at every stream-taking entry point, on the MI355X: each case runs the protocol of tests/streamutil.py
(late inputs behind a delay, an early clobber behind the call, one non-default stream, no host synchronisation) and must
return, bit for bit, what the same call returns on quiescent inputs.  Two controls plant the caller-side defects (a call
that does not wait for its inputs; a reader that does not wait for the call) and must observe them.

B = 3 throughout, synthetic weights, fp16 (bf16 as well for the three plain forwards).  Run with -s for the table of call
time, delay and unit count per case."""
import pytest
import torch

from genconvit_amd import _lib, synth
from tests import streamutil as su

pytestmark = pytest.mark.gpu
torch.set_grad_enabled(False)

B = 3
F16, BF16 = torch.float16, torch.bfloat16
_M = {}              # this module's handles: (kind, dtype, schedule) -> module instance
_IN = {}


def ed(dtype=F16):
    if ("ed", dtype) not in _M:
        _M[("ed", dtype)] = su.fresh(su.base_model("ed", dtype))
    return _M[("ed", dtype)]


def vae(split, monkeypatch, dtype=F16):
    """One VAE handle per (dtype, schedule): GCV_VAE_SPLIT=1, backbone(x) forked to the handle's side stream, or =0, one
    merged pass on the caller's stream (also what the default handle runs inside the ensemble)."""
    key = ("vae", dtype, bool(split))
    if key not in _M:
        _M[key] = su.fresh(su.base_model("vae", dtype), split=bool(split), monkeypatch=monkeypatch, batch=B)
    return _M[key]


def swin(dtype=F16):
    if ("swin", dtype) not in _M:
        _M[("swin", dtype)] = su.fresh(su.base_model("swin", dtype))
    return _M[("swin", dtype)]


def ensemble(m_ed, m_vae):
    from genconvit_amd.model.genconvit import GenConViT
    return GenConViT.from_modules(m_ed, m_vae, net="genconvit")


# true inputs, decoys, second decoys: real frames under three names, three eps draws, three target patterns
NAMES = ("stream.true", "stream.decoy", "stream.decoy2")
TARGETS = ([0, 1, 0], [1, 0, 1], [1, 1, 0])


def xs(dtype=F16, res=224):
    key = ("x", dtype, res)
    if key not in _IN:
        fr = [synth.make_frames(B, name=n) for n in NAMES]
        if res != 224:
            fr = [torch.nn.functional.avg_pool2d(f, 224 // res) for f in fr]
        _IN[key] = [f.to("cuda").to(dtype).contiguous() for f in fr]
    return _IN[key]


def epss():
    if "eps" not in _IN:
        _IN["eps"] = [synth.make_eps(B, name=n).cuda() for n in NAMES]
    return _IN["eps"]


def targets():
    if "t" not in _IN:
        _IN["t"] = [torch.tensor(t, dtype=torch.int32, device="cuda") for t in TARGETS]
    return _IN["t"]


def sets(*groups):
    """[(true, decoy, decoy2) per buffer] -> (inputs, decoys, decoys2)"""
    return tuple([g[k] for g in groups] for k in range(3))


def mk(call, *groups, **kw):
    """A case: (call, inputs, decoys, decoys2, keywords of late_input_early_clobber)."""
    return (call,) + sets(*groups) + (kw,)


# ------------------------------------------------------------------------------------------------ the cases
# Each builder returns (call, inputs, decoys, decoys2, keywords of late_input_early_clobber).
def case_ed_forward(mp, dtype=F16):
    m = ed(dtype)
    return mk(lambda b: m(b[0]), xs(dtype))


def case_ed_explain(mp, layer):
    m = ed()
    return mk(lambda b: m.explain(b[0], target=b[1], upsample=True, layer=layer), xs(), targets())


def _vae_call(m):
    def call(b):
        logits, recon = m(b[0], eps=b[1], want_recon=True, want_mse=True, want_kl=True)
        return logits, recon, m.mse, m.kl
    return call


def case_vae_forward(mp, split, dtype=F16):
    return mk(_vae_call(vae(split, mp, dtype)), xs(dtype), epss())


def case_vae_explain(mp, layer):
    m = vae(True, mp)
    return mk(lambda b: m.explain(b[0], eps=b[1], target=b[2], upsample=True, layer=layer), xs(), epss(), targets())


TAPS = ("vae.bb.stem", "vae.bb.s2.b8", "vae.bb.s3.b2", "vae.bb.pool", "vae.xhat", "vae.feat")


def case_vae_taps(mp):
    """Taps on the backbone stream — its first segment is copied on the handle's side stream — and on two tensors of the
    caller's stream; the tap buffers are the test's, zeroed on the stream before the call and cloned behind it like outputs."""
    from tests import taputil
    m = vae(True, mp)
    h = m._get_handle(B)
    lay = taputil.layout("vae", B)
    bufs = {}
    for name in TAPS:
        n = sum(s[1] * s[2] * s[3] for s in lay[name][1])
        bufs[name] = torch.zeros((n,), dtype=torch.float32 if lay[name][0] else F16, device="cuda")
    inner = _vae_call(m)

    def call(b):
        for name, t in bufs.items():
            t.zero_()
            h.set_tap(name, t)
        try:
            return inner(b), [bufs[n] for n in TAPS]
        finally:
            h.clear_taps()
    return mk(call, xs(), epss())


def case_genconvit_forward(mp, split=False, dtype=F16):
    g = ensemble(ed(dtype), vae(split, mp, dtype))
    return mk(lambda b: g(b[0], eps=b[1]), xs(dtype), epss())


def case_genconvit_explain(mp, layer):
    g = ensemble(ed(), vae(False, mp))
    return mk(lambda b: g.explain(b[0], eps=b[1], target=b[2], upsample=True, layer=layer), xs(), epss(), targets())


def case_convnext_forward(mp):
    m = ed()
    return mk(lambda b: m.backbone_forward(b[0]), xs(F16, 112))


def case_swin_forward(mp):
    m = swin()
    return mk(lambda b: m(b[0]), xs())


# wrapper temporaries: x arrives as a permuted view (the buffer is NHWC), eps in fp16, the target as a Python list, so that
# _prep_input / _check_x, eps.to(float32) / _check_eps and _target create tensors that die when the wrapper returns — while
# the library's streams may still read them.  `temps` names their sizes: the protocol re-allocates and fills those.
def _nhwc():
    if "nhwc" not in _IN:
        _IN["nhwc"] = [x.permute(0, 2, 3, 1).contiguous() for x in xs()]
        _IN["eps16"] = [e.half() for e in epss()]
    return _IN["nhwc"], _IN["eps16"]


TEMPS = (((B, 3, 224, 224), F16), ((B, 12544), torch.float32), ((B,), torch.int32))


def case_temporaries_genconvit_forward(mp):
    g = ensemble(ed(), vae(False, mp))
    return mk(lambda b: g(b[0].permute(0, 3, 1, 2), eps=b[1]), *_nhwc(), temps=TEMPS[:2])


def case_temporaries_vae_explain(mp):
    m = vae(True, mp)
    # torch.as_tensor(list, device=...) is a pageable host-to-device copy on the caller's stream: it may hold the host
    # until the delay is through, so this case reports whether it was armed instead of requiring it
    call = lambda b: m.explain(b[0].permute(0, 3, 1, 2), eps=b[1], target=[0, 1, 0], upsample=True)
    return mk(call, *_nhwc(), temps=TEMPS, must_arm=False)


# launchers: through the C ABI on the current stream, with device-resident arguments (no host-to-device copy in the call).
# Outputs are the test's and are filled with a finite non-zero pattern on the stream first: a memset that landed on the
# null stream would run inside the delay, before that fill, and the kernel's atomics would then add to the pattern.
def _u8(shape, seed):
    g = torch.Generator(device="cuda")
    g.manual_seed(seed)
    return torch.randint(0, 256, shape, dtype=torch.uint8, device="cuda", generator=g)


def _cur():
    return torch.cuda.current_stream().cuda_stream


def case_frame_hist(mp):
    """3 frames of 64 x 96 at R = 2: 12 regions of 32 rows -> S = 4 slices each (csrc/cuts.hip): memset + atomics."""
    lib, (nf, H, W, R) = _lib.load(), (3, 64, 96, 2)

    def call(b):
        out = torch.full((nf, R * R, 64), 7, dtype=torch.int32, device="cuda")
        _lib.check(lib.gcv_frame_hist(b[0].data_ptr(), nf, H, W, R, out.data_ptr(), _cur()), "gcv_frame_hist")
        return out
    return mk(call, [_u8((nf, H, W, 3), k) for k in (11, 12, 13)])


def case_frame_cells(mp):
    """S > 1 needs cell rows of at least 16 pixel rows (H / G / 8 >= 2, csrc/cuts.hip): 3 frames of 128 x 96 at G = 8,
    24 cell rows -> S = 2."""
    lib, (nf, H, W, G) = _lib.load(), (3, 128, 96, 8)

    def call(b):
        out = torch.full((nf, G * G), 7, dtype=torch.int32, device="cuda")
        _lib.check(lib.gcv_frame_cells(b[0].data_ptr(), nf, H, W, G, out.data_ptr(), _cur()), "gcv_frame_cells")
        return out
    return mk(call, [_u8((nf, H, W, 3), k) for k in (21, 22, 23)])


def case_sig_link(mp):
    lib, (n, T) = _lib.load(), (70, 5)                     # two 64-row tiles
    owner = (torch.arange(n, dtype=torch.int32, device="cuda") % T).contiguous()

    def call(b):
        out = torch.full((T, T), 7, dtype=torch.int32, device="cuda")
        _lib.check(lib.gcv_sig_link(b[0].data_ptr(), owner.data_ptr(), n, T, out.data_ptr(), _cur()), "gcv_sig_link")
        return out
    return mk(call, [_u8((n, 384), k) for k in (31, 32, 33)])


def case_vote_windows(mp):
    lib, (nb, nets) = _lib.load(), (37, 2)
    ranges = torch.tensor([[0, 37], [5, 9], [30, 37], [12, 12]], dtype=torch.int32, device="cuda")
    g = torch.Generator(device="cuda")
    g.manual_seed(41)
    logits = [torch.randn((nets * nb, 2), device="cuda", generator=g) for _ in range(3)]

    def call(b):
        fp = torch.full((nb, 2), 7.0, device="cuda")
        mean = torch.full((ranges.shape[0], 2), 7.0, device="cuda")
        _lib.check(lib.gcv_vote_windows(b[0].data_ptr(), nb, nets, ranges.data_ptr(), ranges.shape[0], fp.data_ptr(),
                                        mean.data_ptr(), _cur()), "gcv_vote_windows")
        return fp, mean
    return mk(call, logits)


def case_face_crop_preprocess(mp):
    lib, (nf, H, W, S) = _lib.load(), (3, 64, 96, 32)
    boxes = torch.tensor([[0, 0, 96, 64, 0], [1, 3, 70, 50, 9], [2, 10, 96, 64, 40], [1, 0, 33, 31, 0]], dtype=torch.int32,
                         device="cuda")

    def call(b):
        out = torch.full((boxes.shape[0], 3, S, S), 7.0, dtype=F16, device="cuda")
        _lib.check(lib.gcv_face_crop_preprocess(_lib.GCV_F16, b[0].data_ptr(), nf, H, W, boxes.data_ptr(), boxes.shape[0],
                                                out.data_ptr(), S, _cur()), "gcv_face_crop_preprocess")
        return out
    return mk(call, [_u8((nf, H, W, 3), k) for k in (51, 52, 53)])


# case id -> (the stream-taking entry points it runs, builder).  tests/test_streams_cpu.py holds the union of the entry
# points against streamutil.COVERED.
CASES = {
    "ed_forward[fp16]": (("gcv_ed_forward",), lambda mp: case_ed_forward(mp)),
    "ed_forward[bf16]": (("gcv_ed_forward",), lambda mp: case_ed_forward(mp, BF16)),
    "ed_explain[s3]": (("gcv_ed_explain",), lambda mp: case_ed_explain(mp, "s3")),
    "ed_explain[s2]": (("gcv_ed_explain_at",), lambda mp: case_ed_explain(mp, "s2")),
    "vae_forward[split,fp16]": (("gcv_vae_forward",), lambda mp: case_vae_forward(mp, True)),
    "vae_forward[split,bf16]": (("gcv_vae_forward",), lambda mp: case_vae_forward(mp, True, BF16)),
    "vae_forward[merged,fp16]": (("gcv_vae_forward",), lambda mp: case_vae_forward(mp, False)),
    "vae_explain[split,s2]": (("gcv_vae_explain_at",), lambda mp: case_vae_explain(mp, "s2")),
    "vae_forward[split,taps]": (("gcv_vae_forward",), case_vae_taps),
    "genconvit_forward[fp16]": (("gcv_genconvit_forward",), lambda mp: case_genconvit_forward(mp)),
    "genconvit_forward[bf16,split vae]": (("gcv_genconvit_forward",), lambda mp: case_genconvit_forward(mp, True, BF16)),
    "genconvit_forward[fp16,split vae]": (("gcv_genconvit_forward",), lambda mp: case_genconvit_forward(mp, True)),
    "genconvit_explain[s3]": (("gcv_genconvit_explain",), lambda mp: case_genconvit_explain(mp, "s3")),
    "genconvit_explain[s2]": (("gcv_genconvit_explain_at",), lambda mp: case_genconvit_explain(mp, "s2")),
    "convnext_forward[112]": (("gcv_convnext_forward",), case_convnext_forward),
    "swin_forward": (("gcv_swin_forward",), case_swin_forward),
    "temporaries[genconvit_forward]": (("gcv_genconvit_forward",), case_temporaries_genconvit_forward),
    "temporaries[vae_explain]": (("gcv_vae_explain",), case_temporaries_vae_explain),
    "frame_hist[S>1]": (("gcv_frame_hist",), case_frame_hist),
    "frame_cells[S>1]": (("gcv_frame_cells",), case_frame_cells),
    "sig_link": (("gcv_sig_link",), case_sig_link),
    "vote_windows": (("gcv_vote_windows",), case_vote_windows),
    "face_crop_preprocess": (("gcv_face_crop_preprocess",), case_face_crop_preprocess),
}


@pytest.mark.parametrize("case", list(CASES))
def test_late_inputs_and_an_early_clobber_do_not_change_the_result(case, monkeypatch):
    call, inputs, decoys, decoys2, kw = CASES[case][1](monkeypatch)
    su.late_input_early_clobber(call, inputs, decoys, decoys2, name=case, **kw)


# ------------------------------------------------------------------------------------------------ the controls
CONTROLS = ("ed_forward", "genconvit_forward")


def _control_case(which, mp):
    return case_ed_forward(mp) if which == "ed_forward" else case_genconvit_forward(mp)


@pytest.mark.parametrize("which", CONTROLS)
def test_control_a_call_that_does_not_wait_for_its_inputs_computes_the_decoys(which, monkeypatch):
    """Planted in the caller: the missing fork edge.  Failing here means the delay is too short to show a missing edge, so
    the cases above prove nothing: a construction failure of the test (streamutil.DelayError), never a skip."""
    call, inputs, decoys, _, _ = _control_case(which, monkeypatch)
    seen = su.missing_fork_edge(call, inputs, decoys, name=which)
    print(f"control, missing fork edge, {which}: the unordered call returned {seen}")


@pytest.mark.parametrize("which", CONTROLS)
def test_control_a_reader_that_does_not_wait_for_the_call_sees_the_sentinel(which, monkeypatch):
    """Planted in the caller: the missing join edge, through the C ABI with output buffers the test owns."""
    lib = _lib.load()
    if which == "ed_forward":
        he = ed()._get_handle(B)
        out = torch.empty((B, 2), device="cuda")
        groups = sets(xs())

        def enqueue(b, o, stream):
            _lib.check(lib.gcv_ed_forward(he._h, b[0].data_ptr(), B, o.data_ptr(), stream), "gcv_ed_forward")
    else:
        he, hv = ed()._get_handle(B), vae(False, monkeypatch)._get_handle(B)
        out = torch.empty((2 * B, 2), device="cuda")
        groups = sets(xs(), epss())

        def enqueue(b, o, stream):
            _lib.check(lib.gcv_genconvit_forward(he._h, hv._h, b[0].data_ptr(), b[1].data_ptr(), B, o.data_ptr(), stream),
                       "gcv_genconvit_forward")
    seen = su.missing_join_edge(enqueue, groups[0], groups[1], out, 12345.0, name=which)
    print(f"control, missing join edge, {which}: the unordered read returned {seen}")


# ------------------------------------------------------------------------------------------------ caller stream changes
@pytest.mark.parametrize("which", ["vae_forward[split]", "genconvit_forward"])
def test_back_to_back_calls_from_two_caller_streams(which, monkeypatch):
    """One handle, two calls from two different caller streams, ordered by the caller with wait_stream: the handle's lazily
    created side streams and events are forked from a new stream each time.  The first call runs on the second decoys
    behind the delay, the second on the true inputs; both must equal their baselines."""
    if which == "genconvit_forward":
        call, inputs, decoys, decoys2, _ = case_genconvit_forward(monkeypatch)
    else:
        call, inputs, decoys, decoys2, _ = case_vae_forward(monkeypatch, True)
    bufs = [torch.empty_like(t) for t in inputs]
    base = su._Baselines(call, bufs, (inputs, decoys, decoys2))
    su._distinct(which, base)
    d = su.delay()
    units = d.units_for(base.wall_ms, which)
    for b, v in zip(bufs, decoys):
        b.copy_(v)
    torch.cuda.synchronize()
    s1, s2 = su.streams()[0], su.streams()[2]
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    with torch.cuda.stream(s1):
        e0.record()
        d.enqueue(units)
        e1.record()
        for b, v in zip(bufs, decoys2):
            b.copy_(v)
        first = [o.clone() for o in su.flat(call(bufs))]
    s2.wait_stream(s1)
    with torch.cuda.stream(s2):
        for b, v in zip(bufs, inputs):
            b.copy_(v)
        second = [o.clone() for o in su.flat(call(bufs))]
        for b, v in zip(bufs, decoys):
            b.copy_(v)
        armed = not e1.query()
    s2.synchronize()
    torch.cuda.synchronize()
    measured = e0.elapsed_time(e1)
    su._row("two caller streams: " + which, base.wall_ms, measured, units, armed)
    su._check_delay(which, measured, base.wall_ms)
    assert armed, f"{which}: the test could not build its delay: it ended before both calls were enqueued"
    assert all(torch.equal(a, b) for a, b in zip(first, base.decoy2)), \
        f"{which}: the first call (stream 1, second decoys) equals {base.which(first)}"
    assert all(torch.equal(a, b) for a, b in zip(second, base.true)), \
        f"{which}: the second call (stream 2, true inputs) equals {base.which(second)}"
