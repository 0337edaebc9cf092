"""Stream ordering of the C ABI, checked from the caller's side (tests/test_streams_gpu.py, tests/test_handle_reuse_gpu.py,
tests/test_streams_cpu.py).

include/genconvit_hip.h promises that every call that takes a ``gcv_stream`` enqueues its work after what that stream held
at the call and before what the stream is given next, also where the library forks onto streams of its own.  A test that
hands the library finished inputs and synchronises before it looks cannot see a missing edge.  The protocol here does
neither (``late_input_early_clobber``):

  * the buffers the call reads hold DECOYS — other real frames, another eps, another target class — while, on a
    non-default stream ``s``, a long delay runs, then the true inputs are copied in, then the call is made, its results are
    cloned, the buffers are overwritten with a second set of decoys, and new tensors of the sizes of the wrapper's
    temporaries are allocated and filled (the caching allocator hands out what the wrapper freed on return).  Not one host
    synchronisation in between;
  * ``s.synchronize()``; every clone must be ``torch.equal`` to what the same call gave on quiescent true inputs.

Work that does not wait for ``s`` (a side stream without its fork event, a launch or memset on the null stream, a tap copy
on another stream) runs inside the delay and reads the decoys; a caller stream that does not wait for the library's join
event lets the clones, the second decoys and the re-issued temporaries overtake the library.  Either way the result is
finite and different, and the failure message says which baseline, if any, it equals.

Two controls plant those defects in the CALLER and must observe them, or the delay was too short to show anything:
``missing_fork_edge`` issues the call on a stream that does not wait for ``s`` (it must compute the decoys' result) and
``missing_join_edge`` reads the output buffers from such a stream (it must read the sentinel they were filled with).  All
memory any of this touches is live and correctly sized; all values are finite.

What a pass does not show: freedom from races between two of the library's own streams that both start after the fork and
both end before the join (the arena's layout, the order of the ED and VAE networks inside the ensemble): both sides of such
a race see the true inputs.

This module imports without a GPU: the census (test_streams_cpu.py) reads COVERED / EXEMPT from it.
"""
import copy
import math
import os
import re
import time

import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(REPO, "include", "genconvit_hip.h")

# ------------------------------------------------------------------------------------------------ the census
# Entry points with a gcv_stream parameter that a case of tests/test_streams_gpu.py runs through the protocol.
COVERED = frozenset({
    "gcv_ed_forward", "gcv_vae_forward", "gcv_genconvit_forward",
    "gcv_ed_explain", "gcv_ed_explain_at", "gcv_vae_explain", "gcv_vae_explain_at",
    "gcv_genconvit_explain", "gcv_genconvit_explain_at",
    "gcv_convnext_forward", "gcv_swin_forward",
    "gcv_frame_hist", "gcv_frame_cells", "gcv_sig_link",          # a hipMemsetAsync and a kernel
    "gcv_vote_windows",                                           # two kernels
    "gcv_face_crop_preprocess",                                   # one kernel: the single-launch representative
})

_ONE_LAUNCH = "one kernel launch on the stream argument, nothing else is enqueued (gcv_face_crop_preprocess stands for these)"
_K = "per-kernel test entry: launches on the stream argument only, the kernels the covered forwards enqueue on `cur`"
_TWIN = "twin of a launcher listed here, same launch path with a planning / timing argument"

# Entry points with a gcv_stream parameter that no case runs, each with the reason.
EXEMPT = {
    "gcv_allgather_logits": "RCCL's ncclAllGather on the stream argument; ordering is RCCL's, and one rank makes it a device copy",
    **{n: _ONE_LAUNCH for n in (
        "gcv_preprocess", "gcv_face_crop_resize", "gcv_cam_overlay", "gcv_scan_annotate", "gcv_yuv420_to_rgb",
        "gcv_rgb_to_yuv420", "gcv_track_match", "gcv_track_chain", "gcv_hist_diff", "gcv_hist_diff_lag", "gcv_blend_fit",
        "gcv_face_quality", "gcv_face_signature", "gcv_vote", "gcv_vote_segments")},
    **{n: _K for n in (
        "gcv_k_gemm", "gcv_k_stem_ln", "gcv_k_stem_ln_c", "gcv_k_dwconv7_ln", "gcv_k_dwconv7_ln2", "gcv_k_ln_patchify",
        "gcv_k_layernorm_rows", "gcv_k_pool_ln", "gcv_k_pool_ln_rows", "gcv_k_conv3_first", "gcv_k_convt2_small",
        "gcv_k_reparam", "gcv_k_head_tail", "gcv_k_head_tail_splitk", "gcv_k_resize_mse", "gcv_k_swin_window_attn",
        "gcv_k_patch_merge_ln", "gcv_k_mean_tokens", "gcv_k_head_bwd", "gcv_k_bb_bwd", "gcv_k_cam", "gcv_k_pool_ln_bwd",
        "gcv_k_scale_rows", "gcv_k_gelu_bwd", "gcv_k_dw_ln_bwd", "gcv_k_dw_dgrad_res", "gcv_k_down_ln_bwd", "gcv_k_cam2",
        "gcv_k_fused_mlp", "gcv_k_fused_mlp_lnp")},
    **{n: _TWIN for n in (
        "gcv_k_dwconv7_ln_planned", "gcv_k_dwconv7_ln2_planned", "gcv_k_fused_mlp_planned", "gcv_k_fused_mlp_lnp_planned",
        "gcv_k_fused_mlp_timed")},
}


def stream_entry_points(header_text=None):
    """Names of the functions include/genconvit_hip.h declares with a ``gcv_stream`` parameter, in header order."""
    if header_text is None:
        with open(HEADER) as f:
            header_text = f.read()
    text = re.sub(r"/\*.*?\*/", " ", header_text, flags=re.S)
    text = re.sub(r"//[^\n]*", " ", text)
    out = []
    for m in re.finditer(r"\b(gcv_\w+)\s*\(([^;{}()]*)\)\s*;", text):
        if re.search(r"\bgcv_stream\b", m.group(2)):
            out.append(m.group(1))
    return out


# ------------------------------------------------------------------------------------------------ models and inputs
_BASE = {}


def base_model(kind, dtype):
    """The session's one parameter set of network ``kind`` ("ed", "vae", "swin") in ``dtype`` with the synthetic weights, on
    the device (built like ed_model / vae_model / swin_model of tests/test_parity_gpu.py).  Never called itself: the tests
    run ``fresh(base_model(...))`` copies, each with a handle of its own."""
    from genconvit_amd import spec, synth
    from genconvit_amd.model.config import load_config
    key = (kind, dtype)
    if key not in _BASE:
        if kind == "swin":
            from genconvit_amd.model.swin import SwinTinyEmbedder
            m = SwinTinyEmbedder(init="empty")
            m.load_state_dict(synth.make_state_dict(spec.swin_tiny_spec(""), synth.DEFAULT_SEED, "swin/"))
        else:
            from genconvit_amd.model.genconvit_ed import GenConViTED
            from genconvit_amd.model.genconvit_vae import GenConViTVAE
            from tests.conftest import synthetic_sd
            m = (GenConViTED if kind == "ed" else GenConViTVAE)(load_config(), init="empty")
            m.load_state_dict(synthetic_sd(kind))
        _BASE[key] = m.to("cuda").to(dtype).eval()
    return _BASE[key]


def fresh(model, max_batch=None, split=None, monkeypatch=None, keep_kl_weights=True, batch=None):
    """A new module instance over ``model``'s parameters with NO handle yet: its first call creates and packs a brand-new
    handle (a shallow copy shares the nn.Parameters, which are read-only here; the 2.6 GB VAE state is not rebuilt).
    ``max_batch``: reserve() it.  ``split``: create the handle now, for ``batch`` frames, under GCV_VAE_SPLIT=<split> — the
    library reads the switch when a handle is constructed (fresh_vae of tests/test_parity_gpu.py); None leaves the
    variable unset for the creation (the default: split alone, merged inside the ensemble)."""
    m = copy.copy(model)
    m._handle, m._handle_key, m._dirty, m._sig_params, m._loaded_sig = None, None, True, None, None
    m._max_batch = m._default_max_batch
    if hasattr(m, "keep_kl_weights"):
        m.keep_kl_weights = keep_kl_weights
        m.kl = m.mse = None
    if max_batch is not None:
        m.reserve(max_batch)
    if monkeypatch is not None:
        with monkeypatch.context() as mp:
            if split is None:
                mp.delenv("GCV_VAE_SPLIT", raising=False)
            else:
                mp.setenv("GCV_VAE_SPLIT", "1" if split else "0")
            m._get_handle(batch or 1)
    return m


def flat(outs):
    """The tensors of a call's result — a tensor, or nested tuples / lists / dicts of tensors and None — in a fixed order."""
    if outs is None:
        return []
    if torch.is_tensor(outs):
        return [outs]
    if isinstance(outs, dict):
        return [t for k in sorted(outs) for t in flat(outs[k])]
    return [t for o in outs for t in flat(o)]


# ------------------------------------------------------------------------------------------------ the delay
PAD = 4.0            # delay aimed at: PAD x the call's wall time (the bound that is asserted is FACTOR x) ...
AIM_MS = 30.0        # ... and 30 ms: the unit is timed once, on an idle GPU, and the clocks move (20 units came to 18.4 ... 20.7 ms)
FACTOR = 3.0         # the control's call must be enqueued by the host and finish on the device inside the delay
MIN_MS = 20.0
MAX_MS = 2000.0
# One unit: a 2048^3 fp32 torch.mm into a scratch tensor, about 0.1 ms.  Large enough that the host enqueues units far
# faster than the device retires them; small enough that it leaves most of the 256 CUs to whatever runs beside the delay
# (a unit of 4096^3 held every CU for 1 ms at a time, and a 1 ms forward issued beside it did not finish within 20 ms).
DELAY_N = 2048


class DelayError(AssertionError):
    """The test could not build its delay: a construction failure of the test, not a finding about the library."""


class Delay:
    """Repeated large torch.mm into a scratch tensor on the current stream; the unit is timed once with events."""

    def __init__(self):
        g = torch.Generator(device="cuda")
        g.manual_seed(7)
        self.a = (torch.rand((DELAY_N, DELAY_N), device="cuda", generator=g) - 0.5) * (2.0 / DELAY_N)
        self.b = torch.rand((DELAY_N, DELAY_N), device="cuda", generator=g) - 0.5
        self.c = torch.empty((DELAY_N, DELAY_N), device="cuda")
        self.enqueue(16)                                       # warm-up: kernel selection, clocks
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        self.enqueue(64)
        e1.record()
        e1.synchronize()
        self.unit_ms = e0.elapsed_time(e1) / 64.0

    def enqueue(self, units):
        for _ in range(units):
            torch.mm(self.a, self.b, out=self.c)

    def units_for(self, wall_ms, what):
        need = max(AIM_MS, PAD * wall_ms)
        units = int(math.ceil(need / self.unit_ms))
        if units * self.unit_ms > MAX_MS:
            raise DelayError(f"{what}: the test could not build its delay: {need:.1f} ms wanted ({PAD:g} x the call's "
                             f"{wall_ms:.2f} ms), {units} units of {self.unit_ms:.3f} ms pass {MAX_MS:g} ms")
        return units


_SHARED = {}


def delay():
    if "delay" not in _SHARED:
        _SHARED["delay"] = Delay()
    return _SHARED["delay"]


N_STREAMS = 6


def streams():
    """The non-default streams of these tests.  A case uses one of them, the two-caller case and a control two at a time
    (beside the default stream and the library's own); the others are there for the controls to choose from."""
    if "streams" not in _SHARED:
        _SHARED["streams"] = tuple(torch.cuda.Stream() for _ in range(N_STREAMS))
    return _SHARED["streams"]


TABLE = []           # one row per protocol run, printed by the tests (-s)


def _row(name, wall_ms, delay_ms, units, armed, note=""):
    row = (f"{name:46s} call {wall_ms:7.2f} ms   delay {delay_ms:7.1f} ms = {delay_ms / max(wall_ms, 1e-9):5.1f} x   "
           f"{units:4d} units   enqueued inside the delay: {'yes' if armed else 'NO'}{note}")
    TABLE.append(row)
    print("\n" + row)
    return row


def _check_delay(name, measured_ms, wall_ms):
    if not (measured_ms >= MIN_MS and measured_ms >= FACTOR * wall_ms):
        raise DelayError(f"{name}: the test could not build its delay: it measured {measured_ms:.1f} ms on the stream, the "
                         f"bound is max({MIN_MS:g} ms, {FACTOR:g} x {wall_ms:.2f} ms)")


class _Baselines:
    """call(bufs) on quiescent inputs, default stream, everything synchronised: the true inputs' result, the decoys', the
    second decoys'; and the wall time of one synchronised call (host enqueue + device), after the first as warm-up."""

    def __init__(self, call, bufs, sets):
        self.res, wall = [], []
        for k, vals in enumerate(sets):
            for b, v in zip(bufs, vals):
                b.copy_(v)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            outs = call(bufs)
            torch.cuda.synchronize()
            if k:
                wall.append((time.perf_counter() - t0) * 1e3)
            self.res.append([o.clone() for o in flat(outs)])
        torch.cuda.synchronize()
        self.wall_ms = max(wall)
        self.true, self.decoy = self.res[0], self.res[1]
        self.decoy2 = self.res[2] if len(self.res) > 2 else None

    def which(self, got):
        """Which baseline a result equals, for the failure message."""
        for label, want in (("the true inputs'", self.true), ("the decoys'", self.decoy), ("the second decoys'", self.decoy2)):
            if want is not None and len(want) == len(got) and all(torch.equal(a, b) for a, b in zip(got, want)):
                return label + " baseline"
        per = []
        for i, g in enumerate(got):
            hit = [lab for lab, want in (("true", self.true), ("decoys", self.decoy), ("second decoys", self.decoy2))
                   if want is not None and torch.equal(g, want[i])]
            per.append(f"#{i}: {' / '.join(hit) if hit else 'neither'}")
        return "no baseline as a whole (per returned tensor: " + ", ".join(per) + ")"


def _distinct(name, base):
    """The decoys must be told apart from the true inputs by every returned tensor, or a too-early read would not show."""
    for i, (a, b) in enumerate(zip(base.true, base.decoy)):
        assert not torch.equal(a, b), f"{name}: returned tensor #{i} is the same for the true inputs and the decoys"
    for t in base.true + base.decoy:
        assert bool(torch.isfinite(t.float()).all()), f"{name}: a baseline holds a non-finite value"


def late_input_early_clobber(call, inputs, decoys, decoys2=None, name="call", temps=(), must_arm=True):
    """The protocol of this module's docstring.  ``call(bufs)``: bufs is a list of device tensors shaped like ``inputs``
    (the buffers the entry point reads); returns tensors (nested, None allowed).  ``inputs`` / ``decoys`` / ``decoys2``:
    lists of device tensors of equal shapes (decoys2 defaults to the decoys rolled by one frame).  ``temps``: (shape, dtype)
    of every temporary the wrapper creates and frees inside the call.  ``must_arm``: require that the host had enqueued the
    call and the clobbering before the delay ended on the device (False where the wrapper itself blocks the host, e.g. on
    a pageable host-to-device copy: the case is then reported as not armed instead of failing).
    Returns the baselines (for further checks)."""
    if decoys2 is None:
        decoys2 = [d.roll(1, 0) for d in decoys]
    bufs = [torch.empty_like(t) for t in inputs]
    base = _Baselines(call, bufs, (inputs, decoys, decoys2))
    _distinct(name, base)
    d = delay()
    units = d.units_for(base.wall_ms, name)
    for b, v in zip(bufs, decoys):
        b.copy_(v)
    torch.cuda.synchronize()
    s = streams()[0]
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    with torch.cuda.stream(s):
        e0.record()
        d.enqueue(units)
        e1.record()
        for b, v in zip(bufs, inputs):
            b.copy_(v)
        outs = call(bufs)
        got = [o.clone() for o in flat(outs)]
        for b, v in zip(bufs, decoys2):
            b.copy_(v)
        fills = [torch.full(tuple(shape), 0.5 if dt.is_floating_point else 1, dtype=dt, device="cuda") for shape, dt in temps]
        armed = not e1.query()
    s.synchronize()
    torch.cuda.synchronize()
    measured = e0.elapsed_time(e1)
    _row(name, base.wall_ms, measured, units, armed, "" if must_arm or armed else "  (the wrapper blocks the host)")
    _check_delay(name, measured, base.wall_ms)
    if must_arm and not armed:
        raise DelayError(f"{name}: the test could not build its delay: the delay had ended on the device before the host "
                         "had enqueued the call and the clobbering")
    ok = len(got) == len(base.true) and all(torch.equal(a, b) for a, b in zip(got, base.true))
    assert ok, (f"{name}: enqueued behind late inputs and in front of a clobber on one stream, the call did not give the "
                f"result of its true inputs: it equals {base.which(got)}")
    del fills, outs
    return base




# The runtime maps streams onto a few hardware queues, and two streams that share one run in submission order whatever
# edges the program has or lacks: a call issued on such a neighbour of ``s`` — or one that forks onto a stream of the
# library's that is one — waits behind the delay although nothing tells it to; and a reader that shares a queue with a
# side stream of the library's waits behind that stream's wait for the fork event.  (Seen on the MI355X with 4 hardware
# queues: alone in a process the ensemble controls found their pair at the first to fifth try of three streams; behind
# the rest of the suite no pair of three streams would do.)  A control therefore takes the first (delay stream, third
# stream) pair of this module's streams on which its unordered work does land inside the delay; only when no pair does
# has the test failed to build its delay.  Order: every stream is tried in both roles before one is tried twice.
STREAM_PAIRS = tuple((i, (i + k) % N_STREAMS) for k in range(1, N_STREAMS) for i in range(N_STREAMS))


def _behind_a_delay(units, on_s, on_t, pair):
    """Enqueue the delay and ``on_s()`` on stream pair[0], then ``on_t()`` on pair[1], which does not wait for it; wait for
    pair[1] alone.  Returns (whether the delay was still running then, its length on the stream in ms, on_t's result)."""
    s, t = streams()[pair[0]], streams()[pair[1]]
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    with torch.cuda.stream(s):
        e0.record()
        delay().enqueue(units)
        e1.record()
        on_s()
    with torch.cuda.stream(t):                                 # no t.wait_stream(s): the planted defect
        res = on_t()
    t.synchronize()
    inside = not e1.query()
    torch.cuda.synchronize()                                   # every tensor of the attempt is still referenced here
    return inside, e0.elapsed_time(e1), res


def missing_fork_edge(call, inputs, decoys, name="call"):
    """Control: the caller's defect "the call's stream does not wait for the inputs".  The protocol's first half, with the
    call issued on a third stream that does not wait for ``s``: it runs inside the delay, reads the decoys the buffers
    still hold, and must return exactly the decoys' baseline.  Anything else means the delay was too short."""
    bufs = [torch.empty_like(t) for t in inputs]
    base = _Baselines(call, bufs, (inputs, decoys))
    _distinct(name, base)
    units = delay().units_for(base.wall_ms, name)

    def late_inputs():
        for b, v in zip(bufs, inputs):
            b.copy_(v)

    def unordered_call():
        outs = call(bufs)
        return outs, [o.clone() for o in flat(outs)]
    for tries, pair in enumerate(STREAM_PAIRS, 1):
        for b, v in zip(bufs, decoys):
            b.copy_(v)
        torch.cuda.synchronize()
        inside, measured, (outs, got) = _behind_a_delay(units, late_inputs, unordered_call, pair)
        _row("control, missing fork edge: " + name, base.wall_ms, measured, units, inside, f"  (streams {pair}, try {tries})")
        _check_delay(name, measured, base.wall_ms)
        if inside:
            break
    else:
        raise DelayError(f"{name}: the test could not build its delay: on none of the {len(STREAM_PAIRS)} stream pairs had the "
                         f"unordered call finished when the delay ended ({measured:.1f} ms for a call of {base.wall_ms:.2f} ms)")
    seen = base.which(got)
    if seen != "the decoys' baseline":
        raise DelayError(f"{name}: the test could not build its delay: a call that does not wait for its inputs finished "
                         f"inside the delay and yet returned {seen}")
    return seen


def missing_join_edge(enqueue, inputs, decoys, out, sentinel, name="call"):
    """Control: the caller's defect "the reader does not wait for the call's stream".  ``enqueue(bufs, out, stream_ptr)``
    issues the entry point through the C ABI on the stream with that handle, writing into ``out``, a buffer of the test's
    that holds ``sentinel`` everywhere.  The call is issued correctly on ``s`` behind the delay; a third stream that does
    not wait for ``s`` copies ``out`` and must find the sentinel.  Returns what it read."""
    bufs = [torch.empty_like(t) for t in inputs]
    dflt = torch.cuda.current_stream().cuda_stream

    def call(bs):
        out.fill_(sentinel)
        enqueue(bs, out, dflt)
        return out
    base = _Baselines(call, bufs, (inputs, decoys))
    _distinct(name, base)
    assert not bool((base.true[0] == sentinel).any()), f"{name}: the sentinel occurs in the result"
    units = delay().units_for(base.wall_ms, name)

    def ordered_call():
        for b, v in zip(bufs, inputs):
            b.copy_(v)
        enqueue(bufs, out, torch.cuda.current_stream().cuda_stream)
    for tries, pair in enumerate(STREAM_PAIRS, 1):
        for b, v in zip(bufs, decoys):
            b.copy_(v)
        out.fill_(sentinel)
        torch.cuda.synchronize()
        inside, measured, early = _behind_a_delay(units, ordered_call, out.clone, pair)
        _row("control, missing join edge: " + name, base.wall_ms, measured, units, inside, f"  (streams {pair}, try {tries})")
        _check_delay(name, measured, base.wall_ms)
        assert torch.equal(out, base.true[0]), f"{name}: the ordered call itself gave {base.which([out])}"
        if inside:
            break
    else:
        raise DelayError(f"{name}: the test could not build its delay: on none of the {len(STREAM_PAIRS)} stream pairs was the "
                         "unordered read through before the delay ended")
    if not bool((early == sentinel).all()):
        raise DelayError(f"{name}: the test could not build its delay: a read that does not wait for the call's stream did "
                         "not find the sentinel")
    return "the sentinel"
