"""Builders for the ten Grad-CAM backward kernels (csrc/cam.hip, csrc/cam_bwd.hip), on kcases.Case / kcases.MultiCase: the
CPU inputs of a case exactly as tests/test_cam_kernels_gpu.py uploads them (fp32 tensors holding values of the storage dtype T
wherever the kernel reads T), a float64 reference, one comparator per output, an honest float32 model and the planted defects.
tests/test_kernel_sensitivity_cpu.py audits them without a GPU.

Reference.  A backward kernel's reference is torch autograd in float64 through the forward operation on the case's inputs:
F.conv2d with groups = C, F.layer_norm, F.gelu, the mean over tokens, F.linear, space-to-depth.  The closed forms (LayerNorm
backward, flipped-tap correlation, Phi(x) + x phi(x)) serve the defects and the float32 model only; each builder keeps
`closed64`, the closed form in float64, and the audit shows that it equals the autograd reference to 1e-12.  scale_rows, the
row scaling of gelu_bwd, cam2's mean / dot product and the bilinear upsample are forward operations and are referenced as such
(F.interpolate for the upsample).  The builders switch autograd on for themselves: test modules here switch it off globally.

Comparator (class Part), per output:
  scaled   fp32 outputs: |got - want| <= e s, s a float64 scale per element or row that the builder supplies: for a contraction
           or dot product the sum of the absolute values of the element's terms, for the LayerNorm backwards the row's largest
           |want|.  Where s is 0 the result must equal the reference exactly: ReLU'-killed elements of head_bwd, the rows and
           columns that down_ln_bwd zeroes, and every sentinel-filled gap of an output buffer (the reference holds the sentinel
           there, so a write into a gap fails the comparison).
  T        the two outputs in the storage dtype (scale_rows' out, gelu_bwd's pre): 0.5 ulp_T(want) + e; exact where the
           scaled input is exactly 0
  exact    inv / inv_out: the reference's power of two
e is kcases.E[(family, dtype)], at most 2e-5 (asserted on every comparison).

Inputs.  Vectors are kcases.signed: LayerNorm weight +-[0.5, 1], taps +-[0.05, 0.15], depthwise bias and gamma +-[0.25, 0.5].
The builders assert, in float64 and on the inputs: every scaled row's largest magnitude in [0.55, 0.95] x 2^m (scale_rows,
gelu_bwd); at least a quarter of each map's positions above and a quarter below 0 before the ReLU (cam, cam2; maps of four
positions or more, see below; the builder takes the first of its seeded input sets that has the property); hidden and backbone pre-activations of a ReLU head at least 1e-3 from 0 apart from the planted
zeros; logit margins of at least 0.1 apart from the planted tie.

Defects that cannot exist at a case are left out there (every other entry of the family's catalogue applies):
  one image / one row        image before, frame before, row before, inv / exponent / dh of the row before
  one pass                   dpool row taken as (pass, b) (also one image), upsample of the other pass, passes swapped, tok0 ignored
  one token (hw = 1)         token left out of the mean, 1 / hw missing, first token written alone; the upsample without the half-
                             pixel offset and with x / y swapped (every pixel is the one map value).  Without eps the LayerNorm
                             backward is orthogonal to the pooled row; at hw = 1 cam's one value is rstd sum(dy xc) eps / (var + eps),
                             which the image of eps-sized variance keeps away from 0.  A map of fewer than four positions must
                             have one above 0 in place of the sign balance; where no map of a case has a value below 0 (the
                             one-token cam case) the omitted ReLU is left out
  side 1                     taps flipped, ky / kx transposed, clamped edge (only the centre tap is on data)
  even side                  odd row / column left non-zero
  h2 = 1                     row3 formed with side2 for h2; one patch row and one image: inv indexed by the stage-2 token
  ReLU head                  act' evaluated at act(h) (ReLU'(ReLU(h)) = ReLU'(h)), GELU' without its x phi(x) term
  GELU head                  ReLU'(0) = 1
  no tie / target given      tie resolved to class 1;  target null: target ignored
  constant depthwise bias    bias omitted (LayerNorm removes a constant shift)
  variance far from eps      eps omitted moves a result by 5e-7 of itself: it is planted where a row's variance is of eps' size
                             (image 0 of every pool_ln_bwd / cam case, token 0 of every down_ln_bwd case, the constant-bias
                             case of dw_ln_bwd)
  cam224 null                the three upsample defects
  gamma null                 gamma omitted and its three vec_variants
  dw_dgrad_res               fp32 in every storage dtype: one comparator entry, (family, F32)
Where a defect names "one" tap it is the centre tap of the last channel; the index defects (K index dropped) zero that row
of the weight.
"""
import math

import torch
import torch.nn.functional as F

from tests import kcases, numutil
from tests.kcases import F16, BF16, F32, NAMES, q, round_to, signed, vec_variants, _with
from tests.kutil import rnd

SENT = 7.0
EPS = 1e-6
E_MAX = 2e-5                 # kutil.tol's fp32 figure: no bound here is looser than the project's fp32 gate
T_MAX = {F16: 65504.0, BF16: float(torch.finfo(torch.bfloat16).max), F32: float(torch.finfo(torch.float32).max)}


# ----------------------------------------------------------------------------- comparator
class Part(kcases.Case):
    """one output's comparator: kind "scaled" (scale: float64, broadcastable to the output), "T" (exact: bool mask of the
    elements that must match exactly) or "exact" """

    def __init__(self, family, dtype, kind, what, scale=None, exact=None):
        self.family, self.dtype, self.kind, self.scale, self.exact = family, dtype, kind, scale, exact
        self.what = f"{what} {NAMES[dtype]}"
        self.e = kcases.E[(family, dtype)]
        self.tol_before = E_MAX
        self.bound = None

    def measure(self, got, want):
        """err: largest |got - want|; ratio: largest err / bound (inf where an element that must match exactly does not);
        excess: the quantity E is set from — scaled: largest err / s, T: largest err - 0.5 ulp_T(want), exact: 0 or inf"""
        assert self.e <= E_MAX, f"{self.what}: e = {self.e:.2e} above {E_MAX:.0e}"
        w = want.double()
        g = got.detach().cpu().double().reshape(w.shape)
        err = (g - w).abs()
        err = torch.where(torch.isfinite(err), err, torch.full_like(err, math.inf))
        if self.kind == "scaled":
            s = self.scale.double().expand_as(w)
            bound = self.e * s
            rel = torch.where(s > 0, err / s.clamp(min=1e-300), torch.zeros_like(err))
            excess = rel.max().item()
        elif self.kind == "T":
            half = 0.5 * numutil.ulp(w, self.dtype)
            bound = half + self.e
            if self.exact is not None:
                bound = torch.where(self.exact.expand_as(w), torch.zeros_like(bound), bound)
            excess = (err - half).max().item()
        else:
            bound = torch.zeros_like(err)
            excess = 0.0 if err.max().item() == 0 else math.inf
        ratio = torch.where(bound > 0, err / bound.clamp(min=1e-300),
                            torch.where(err == 0, torch.zeros_like(err), torch.full_like(err, math.inf)))
        i = int(ratio.reshape(-1).argmax())
        return {"err": err.max().item(), "ratio": ratio.reshape(-1)[i].item(), "at": i, "excess": excess,
                "bound": bound.reshape(-1)[i].item()}

    def check(self, got, want, inputs=None):
        m = self.measure(got, want)
        idx = tuple(int(i) for i in torch.unravel_index(torch.tensor(m["at"]), want.shape)) if want.dim() else ()
        msg = (f"{self.what} [{self.kind}]: max |diff| {m['err']:.3e}, worst err/bound {m['ratio']:.2f} at {idx} (bound there "
               f"{m['bound']:.3e}), excess {m['excess']:.3e} (e = {self.e:.1e})")
        return m["ratio"] <= 1.0, msg

    def to_storage(self, t64):
        return round_to(t64, self.dtype) if self.kind == "T" else t64.float().double()


def _case(family, what, dtype, inp, want, kinds, closed, defects):
    """kinds: output -> ("scaled", s) | ("T", exact mask) | ("exact",).  closed(i, f, **flags) -> output -> tensor in dtype f.
    The reference `want` (autograd, float64) is computed once by the builder and shared by everything that uses the case."""
    parts = {}
    for name, k in kinds.items():
        parts[name] = Part(family, dtype, k[0], f"{what} {name}", scale=k[1] if k[0] == "scaled" else None,
                           exact=k[1] if k[0] == "T" else None)

    def model(i):
        out = closed(i, torch.float32)
        return {n: (round_to(v.double(), dtype) if kinds[n][0] == "T" else v.float().double()) for n, v in out.items()}

    case = kcases.MultiCase(what, dtype, inp, lambda i: want, model, defects, parts)
    case.family = family
    case.closed64 = lambda: closed(inp, torch.float64)
    case.scales = {n: k[1] for n, k in kinds.items() if k[0] == "scaled"}
    return case


def _f(i, f):
    return {k: (v.to(f) if torch.is_tensor(v) and v.is_floating_point() else v) for k, v in i.items()}


def _prev_last(t):
    """the last entry along dim 0 takes the entry before it"""
    t = t.clone()
    t[-1] = t[-2]
    return t


# ----------------------------------------------------------------------------- closed forms
def gelu_grad(x, no_xphi=False, phi_only=False, abs_terms=False):
    """Phi(x) + x phi(x) in x's dtype (erfc keeps the negative tail); abs_terms: Phi(x) + |x| phi(x), the scale of a sum that
    cancels near x = -0.75"""
    Phi = 0.5 * torch.special.erfc(-x * (1.0 / math.sqrt(2.0)))
    if no_xphi or phi_only:
        return Phi
    return Phi + (x.abs() if abs_terms else x) * (1.0 / math.sqrt(2.0 * math.pi)) * torch.exp(-0.5 * x * x)


def act_grad(x, act, at_zero=0.0, no_xphi=False, abs_terms=False):
    if act == 2:
        return gelu_grad(x, no_xphi=no_xphi, abs_terms=abs_terms)
    return torch.where(x > 0, torch.ones_like(x), torch.where(x == 0, torch.full_like(x, at_zero), torch.zeros_like(x)))


def act_fwd(x, act):
    return F.gelu(x) if act == 2 else F.relu(x)


def ln_bwd(y, dy, eps, no_mean=False, no_proj=False, no_rstd=False, no_eps=False):
    """LayerNorm backward over the last dimension: y the LayerNorm's input, dy = d out * weight"""
    xc = y - y.mean(-1, keepdim=True)
    rstd = 1.0 / torch.sqrt((xc * xc).mean(-1, keepdim=True) + (0.0 if no_eps else eps))
    xh = xc * rstd
    mdy = 0.0 if no_mean else dy.mean(-1, keepdim=True)
    mdyx = 0.0 if no_proj else (dy * xh).mean(-1, keepdim=True)
    return (1.0 if no_rstd else rstd) * (dy - mdy - xh * mdyx)


def upsample(m, half=True, swap=False):
    """(B, S, S) -> (B, 224, 224), bilinear, align_corners = False, as the kernels do it: lerp along x, then along y"""
    S, f = m.shape[-1], m.dtype
    o = torch.arange(224, dtype=f)
    src = ((o + 0.5) * (S / 224.0) - 0.5).clamp(min=0) if half else o * (S / 224.0)
    i0 = src.floor().long().clamp(max=S - 1)
    i1 = (i0 + 1).clamp(max=S - 1)
    l = src - i0.to(f)
    if swap:
        m = m.transpose(1, 2)
    r = m[:, :, i0] * (1 - l) + m[:, :, i1] * l
    return r[:, i0, :] * (1 - l)[:, None] + r[:, i1, :] * l[:, None]


def _balanced(pre):
    """ReLU sign balance of one map before the ReLU: at least a quarter of its positions above 0 and a quarter below; a map of
    fewer than four positions has one above 0 (else the ReLU would hide every defect there)"""
    n = pre.numel()
    if n < 4:
        return bool((pre > 0).any())
    return bool((pre > 0).sum() * 4 >= n and (pre < 0).sum() * 4 >= n)


def _search(make, maps, what):
    """the first of the seeded input sets make(attempt) whose maps(inputs), (B, hw) pre-ReLU values per pass, are all balanced:
    a condition on the inputs, checked on the float64 reference"""
    for attempt in range(64):
        inp = make(attempt)
        if all(_balanced(m[b]) for m in maps(inp) for b in range(m.shape[0])):
            return inp
    raise AssertionError(f"{what}: no input set with balanced map signs")


# ----------------------------------------------------------------------------- head_bwd
@torch.enable_grad()
def head_bwd(B, S, act, target, dtype, tie=False, zeros=False):
    """target logit -> fc2^T -> act'(hidden) -> fc^T (500 -> 2000) -> act'(backbone logits): dfeat (B, 2000).  target: None,
    "ones" or "mixed".  tie: row B - 1 has equal logits (class 0).  zeros (ReLU): hidden unit 7 has every partial and b1 exactly
    0, and bb_pre[0, 5] is exactly 0."""
    K, N = 500, 2000
    partial = rnd((S, B, K), 1, 1.0 / math.sqrt(S))
    b1 = signed((K,), 2, 0.05, 0.2)
    fc2_w = signed((2, K), 3, 0.5, 1.0) / math.sqrt(K)
    logits = rnd((B, 2), 4, 2.0)
    logits[:, 1] = logits[:, 0] + torch.where(rnd((B,), 5) > 0, 1.0, -1.0) * (0.1 + rnd((B,), 6).abs())
    if tie:
        logits[B - 1, 1] = logits[B - 1, 0]
    fc_w = q(rnd((K, N), 7, 1.0 / math.sqrt(N)), dtype)
    bb_pre = rnd((B, N), 8, 2.0)
    bb_pre[:, [1984, 1999]] = bb_pre[:, [1984, 1999]].abs() + 0.25       # a dropped column shows under either activation
    bb_pre = q(bb_pre, dtype)
    if act == 1:
        bb_pre = torch.where(bb_pre.abs() < 1e-3, torch.full_like(bb_pre, 0.5), bb_pre)
        h = (b1.double() + partial.double().sum(0))
        partial[0] += torch.where(h.abs() < 1e-2, torch.sign(h + (h == 0)) * 0.05, torch.zeros_like(h)).float()
    if zeros:
        partial[:, :, 7], b1[7], bb_pre[0, 5] = 0.0, 0.0, 0.0
    tgt = None
    if target == "ones":
        tgt = torch.ones(B, dtype=torch.int32)
    elif target == "mixed":
        tgt = (torch.arange(B) % 3 == 0).to(torch.int32) * 5          # any value != 0 selects class 1
        tgt[0] = 0 if logits[0, 1] > logits[0, 0] else 5            # row 0 against its argmax: "target ignored" shows
    inp = {"partial": partial, "b1": b1, "fc2_w": fc2_w, "logits": logits, "fc_w": fc_w, "bb_pre": bb_pre}
    if tgt is not None:
        inp["target"] = tgt
    # conditions on the inputs
    h64 = b1.double() + partial.double().sum(0)
    d = (logits[:, 1] - logits[:, 0]).abs().double()
    assert ((d >= 0.1 - 1e-6) | (d == 0)).all() and int((d == 0).sum()) == int(tie)
    if act == 1:
        hz, pz = h64.abs() < 1e-3, bb_pre.abs() < 1e-3
        assert int(hz.sum()) == (B if zeros else 0) and (not zeros or (h64[:, 7] == 0).all())
        assert int(pz.sum()) == int(zeros) and (not zeros or bb_pre[0, 5] == 0)

    def classes(i, swapped=False, tie_to_1=False, ignore_target=False):
        lg = i["logits"]
        t = (lg[:, 1] >= lg[:, 0]) if tie_to_1 else (lg[:, 1] > lg[:, 0])
        if "target" in i and not ignore_target:
            t = i["target"] != 0
        return (~t if swapped else t).long()

    def closed(i, f, cls=None, at_act=False, no_b1=False, no_last_slab=False, no_outer=False, frame_before=False,
               no_xphi=False, at_zero=0.0, col_dropped=None, want_scale=False):
        d = _f(i, f)
        slabs = d["partial"][:S - 1] if no_last_slab else d["partial"]
        h = slabs.sum(0) + (0.0 if no_b1 else d["b1"])
        if at_act:
            h = act_fwd(h, act)
        t = classes(i, **(cls or {}))
        a = d["fc2_w"][t] * act_grad(h, act, at_zero, no_xphi, abs_terms=want_scale)                     # (B, K)
        outer = torch.ones_like(d["bb_pre"]) if no_outer else act_grad(d["bb_pre"], act, at_zero, no_xphi, abs_terms=want_scale)
        if want_scale:
            return (a.abs() @ d["fc_w"].abs()) * outer.abs()
        y = (a @ d["fc_w"]) * outer
        if frame_before:
            y = _prev_last(y)
        if col_dropped is not None:
            y = y.clone()
            y[:, col_dropped] = 0
        return {"dfeat": y}

    # the reference: autograd through act -> F.linear -> act -> fc2's row, the hidden pre-activation pinned to the forward's
    # own split-K sum h0 = b1 + sum of the partials
    z = bb_pre.double().requires_grad_(True)
    feat = act_fwd(z, act)
    hid = h64 + F.linear(feat - feat.detach(), fc_w.double())
    t = classes(inp)
    logit = (act_fwd(hid, act) * fc2_w.double()[t]).sum()
    want = {"dfeat": torch.autograd.grad(logit, z)[0].detach()}
    s = closed(inp, torch.float64, want_scale=True)

    def k_dropped(k):
        def fn(i):
            w = i["fc_w"].clone()
            w[k] = 0
            return closed(_with(i, fc_w=w), torch.float64)
        return fn

    D = lambda **kw: (lambda i: closed(i, torch.float64, **kw))
    defects = {f"k_{k}_dropped": k_dropped(k) for k in (0, 127, 128, 499)}
    defects.update({"column_1999_dropped": D(col_dropped=1999), "column_1984_dropped": D(col_dropped=1984),
                    "class_swapped": D(cls={"swapped": True}), "b1_omitted": D(no_b1=True),
                    "last_slab_omitted": D(no_last_slab=True), "outer_act_grad_omitted": D(no_outer=True)})
    if tie and tgt is None:
        defects["tie_resolved_to_class_1"] = D(cls={"tie_to_1": True})
    if tgt is not None:
        defects["target_ignored"] = D(cls={"ignore_target": True})
    if B > 1:
        defects["frame_before"] = D(frame_before=True)
    if act == 2:
        defects["act_grad_at_act_of_h"] = D(at_act=True)
        defects["gelu_grad_without_x_phi"] = D(no_xphi=True)
    elif zeros:
        defects["relu_grad_at_0_is_1"] = D(at_zero=1.0)
    case = _case("head_bwd", f"head_bwd B={B} S={S} act={act} target={target}" + (" tie" if tie else "") +
                 (" zeros" if zeros else ""), dtype, inp, want, {"dfeat": ("scaled", s)}, closed, defects)
    case.p = {"B": B, "S": S, "act": act}
    return case


# ----------------------------------------------------------------------------- bb_bwd
@torch.enable_grad()
def bb_bwd(rows, C, dtype):
    """dpool (rows, C) = dfeat (rows, 1000) . W, W = head.fc.weight (1000, C) in T"""
    K = 1000
    inp = {"dfeat": rnd((rows, K), 1), "W": q(rnd((K, C), 2, 1.0 / math.sqrt(C)), dtype)}

    def closed(i, f, col_dropped=False, row_before=False):
        d = _f(i, f)
        y = d["dfeat"] @ d["W"]
        if row_before:
            y = _prev_last(y)
        if col_dropped:
            y = y.clone()
            y[:, C - 1] = 0
        return {"dpool": y}

    x = torch.zeros((rows, C), dtype=torch.float64, requires_grad=True)
    want = {"dpool": torch.autograd.grad(F.linear(x, inp["W"].double()), x, inp["dfeat"].double())[0]}
    s = inp["dfeat"].double().abs() @ inp["W"].double().abs()

    def k_dropped(k):
        def fn(i):
            w = i["W"].clone()
            w[k] = 0
            return closed(_with(i, W=w), torch.float64)
        return fn

    defects = {f"k_{k}_dropped": k_dropped(k) for k in (0, 251, 252, 999)}
    defects["last_column_dropped"] = lambda i: closed(i, torch.float64, col_dropped=True)
    if rows > 1:
        defects["row_before"] = lambda i: closed(i, torch.float64, row_before=True)
    case = _case("bb_bwd", f"bb_bwd rows={rows} C={C}", dtype, inp, want, {"dpool": ("scaled", s)}, closed, defects)
    case.p = {"rows": rows, "C": C}
    return case


# ----------------------------------------------------------------------------- pool_ln_bwd and cam
def _pool_inputs(C, hws, B, dtype):
    """stage-3 tokens per pass, LayerNorm weight, dpool (B, npass, C).  Image 0 of every pass is scaled down until the variance
    of its pooled row over the channels is of eps' size (the device of kcases.pool_ln)."""
    def make(attempt):
        inp = {"lnw": signed((C,), 4, 0.5, 1.0), "dpool": rnd((B, len(hws), C), 5 + 100 * attempt)}
        for p, hw in enumerate(hws):
            x = rnd((B, hw, C), 10 + p + 100 * attempt, 2.0)
            x[0] *= 6e-4 * math.sqrt(hw)
            inp[f"A{p}"] = q(x, dtype)
            var = inp[f"A{p}"][0].double().mean(0).var(unbiased=False).item()
            assert 0.3 * EPS <= var <= 3 * EPS, f"pooled variance of image 0, pass {p}: {var:.2e}"
        return inp

    def maps(inp):
        return [(dA * inp[f"A{p}"].double()).sum(-1) for p, dA in enumerate(_pool_autograd(inp, hws))]

    return _search(make, maps, f"pool C={C} hw={hws} B={B}")


def _pool_g(i, f, p, hw, lnw=None, drop_token=False, dpool_pb=False, image_before=False, **ln):
    """g / hw (B, C) of pass p in dtype f, closed form"""
    d = _f(i, f)
    A, dp = d[f"A{p}"], d["dpool"]
    B, npass = dp.shape[0], dp.shape[1]
    m = (A[:, :hw - 1].sum(1) if drop_token else A.sum(1)) * (1.0 / hw)
    rows = dp.reshape(B * npass, -1)[[p * B + b for b in range(B)]] if dpool_pb else dp[:, p]
    w = d["lnw"] if lnw is None else lnw.to(f)
    no_inv = ln.pop("no_inv", False)
    g = ln_bwd(m, rows * w, EPS, **ln) * (1.0 if no_inv else 1.0 / hw)
    return _prev_last(g) if image_before else g


@torch.enable_grad()
def _pool_autograd(inp, hws):
    """autograd through mean over the tokens -> F.layer_norm: d A per pass (B, hw, C), float64"""
    out = []
    for p, hw in enumerate(hws):
        A = inp[f"A{p}"].double().requires_grad_(True)
        y = F.layer_norm(A.mean(1), (A.shape[-1],), inp["lnw"].double(), None, EPS)
        out.append(torch.autograd.grad(y, A, inp["dpool"][:, p].double())[0])
    return out


def _ln_flag_defects(mk):
    return {"mean_dy_term_dropped": mk(no_mean=True), "projection_term_dropped": mk(no_proj=True), "eps_omitted": mk(no_eps=True)}


def pool_ln_bwd(C, hws, B, dtype, tok0=None):
    """pooled LayerNorm2d backward + average-pool backward: dA (M, C) fp32, pass p's image b at rows tok0[p] + b hw[p]; rows that
    belong to no pass keep the sentinel"""
    npass = len(hws)
    tok0 = tok0 or [sum(B * h for h in hws[:p]) for p in range(npass)]
    M = max(tok0[p] + B * hws[p] for p in range(npass)) + 1
    inp = _pool_inputs(C, hws, B, dtype)

    def place(gs, f, first_only=False, no_tok0=False):
        out = torch.full((M, C), SENT, dtype=f)
        for p, hw in enumerate(hws):
            t0 = 0 if (no_tok0 and p == 1) else tok0[p]
            rows = gs[p] if gs[p].dim() == 3 else gs[p][:, None, :].expand(B, hw, C)
            for b in range(B):
                n = 1 if first_only else hw
                out[t0 + b * hw:t0 + b * hw + n] = rows[b, :n]
        return out

    def closed(i, f, first_only=False, no_tok0=False, **kw):
        return {"dA": place([_pool_g(i, f, p, hw, **dict(kw)) for p, hw in enumerate(hws)], f, first_only, no_tok0)}

    dA = _pool_autograd(inp, hws)
    want = {"dA": place(dA, torch.float64)}
    s = place([d.abs().amax(-1, keepdim=True).expand_as(d) for d in dA], torch.float64)
    s = torch.where(want["dA"] == SENT, torch.zeros_like(s), s)
    mk = lambda **kw: (lambda i: closed(i, torch.float64, **kw))
    defects = _ln_flag_defects(mk)
    defects.update({"inv_hw_missing": mk(no_inv=True), "ln_w_omitted": mk(lnw=torch.ones(C))})
    for name, v in vec_variants(inp["lnw"]).items():
        defects[f"ln_w_{name}"] = mk(lnw=v)
    if max(hws) > 1:
        defects["one_token_left_out_of_the_mean"] = mk(drop_token=True)
        defects["first_token_written_alone"] = mk(first_only=True)
    if min(hws) == 1 and max(hws) == 1:
        del defects["inv_hw_missing"]
    if B > 1 and npass > 1:
        defects["dpool_row_as_pass_b"] = mk(dpool_pb=True)
    if B > 1:
        defects["image_before"] = mk(image_before=True)
    if npass > 1:
        defects["tok0_ignored"] = mk(no_tok0=True)
    case = _case("pool_ln_bwd", f"pool_ln_bwd C={C} hw={hws} B={B} tok0={tok0}", dtype, inp, want, {"dA": ("scaled", s)},
                 closed, defects)
    case.p = {"C": C, "hws": hws, "B": B, "tok0": tok0, "M": M}
    return case


def cam(C, sides, B, dtype, up_pass=0, with224=True, gap=3):
    """LayerNorm2d backward on the pooled row -> g, CAM = ReLU(sum_c g_c A_c) per stage-3 token, optional 224 x 224 upsample of
    pass up_pass.  `cam` is the whole (B, cam_ld) buffer: pass p's map at off[p], `gap` sentinel elements behind each map."""
    hws = [s * s for s in sides]
    npass = len(sides)
    off = [sum(h + gap for h in hws[:p]) for p in range(npass)]
    cam_ld = off[-1] + hws[-1] + gap
    inp = _pool_inputs(C, hws, B, dtype)

    def closed(i, f, relu=True, half=True, swap=False, other_pass=False, want_scale=False, **kw):
        d = _f(i, f)
        out = torch.full((B, cam_ld), 0.0 if want_scale else SENT, dtype=f)
        maps = []
        for p, hw in enumerate(hws):
            g = _pool_g(i, f, p, hw, **dict(kw))
            A = d[f"A{p}"]
            if kw.get("image_before"):
                A = _prev_last(A)
            pre = (A.abs() * g.abs()[:, None, :]).sum(-1) if want_scale else (A * g[:, None, :]).sum(-1)
            m = pre.clamp(min=0) if relu else pre
            out[:, off[p]:off[p] + hw] = m
            maps.append((m, pre))
        res = {"cam": out}
        if with224:
            up = (1 - up_pass) if other_pass else up_pass
            res["cam224"] = upsample(maps[up][0].reshape(B, sides[up], sides[up]), half, swap)
        return res

    dA = _pool_autograd(inp, hws)
    want, any_negative = {"cam": torch.full((B, cam_ld), SENT, dtype=torch.float64)}, False
    for p, hw in enumerate(hws):
        pre = (dA[p] * inp[f"A{p}"].double()).sum(-1)
        any_negative = any_negative or bool((pre < 0).any())
        want["cam"][:, off[p]:off[p] + hw] = pre.clamp(min=0)
    sc = closed(inp, torch.float64, want_scale=True, relu=False)
    kinds = {"cam": ("scaled", sc["cam"])}
    if with224:
        S = sides[up_pass]
        m = want["cam"][:, off[up_pass]:off[up_pass] + S * S].reshape(B, 1, S, S)
        want["cam224"] = F.interpolate(m, size=(224, 224), mode="bilinear", align_corners=False)[:, 0]
        kinds["cam224"] = ("scaled", sc["cam224"])

    mk = lambda **kw: (lambda i: closed(i, torch.float64, **kw))
    defects = _ln_flag_defects(mk)
    defects.update({"inv_hw_missing": mk(no_inv=True), "ln_w_omitted": mk(lnw=torch.ones(C))})
    if any_negative:
        defects["relu_omitted"] = mk(relu=False)
    for name, v in vec_variants(inp["lnw"]).items():
        defects[f"ln_w_{name}"] = mk(lnw=v)
    if max(hws) > 1:
        defects["one_token_left_out_of_the_mean"] = mk(drop_token=True)
    else:
        del defects["inv_hw_missing"]
    if B > 1 and npass > 1:
        defects["dpool_row_as_pass_b"] = mk(dpool_pb=True)
    if B > 1:
        defects["image_before"] = mk(image_before=True)
    if with224:
        if sides[up_pass] > 1:
            defects["upsample_without_half_pixel_offset"] = mk(half=False)
            defects["upsample_x_y_swapped"] = mk(swap=True)
        if npass > 1:
            defects["upsample_of_the_other_pass"] = mk(other_pass=True)
    case = _case("cam", f"cam C={C} sides={sides} B={B} up_pass={up_pass if with224 else None}", dtype, inp, want, kinds,
                 closed, defects)
    case.p = {"C": C, "sides": sides, "hws": hws, "B": B, "up_pass": up_pass, "with224": with224, "off": off, "cam_ld": cam_ld}
    return case


# ----------------------------------------------------------------------------- scale_rows and gelu_bwd
def row_exp(mx):
    """the exponent e with mx 2^e in [0.5, 1), 0 for a zero row, clamped to +-120: (rows,) float64 in, long out"""
    _, ex = torch.frexp(mx)
    return torch.where(mx > 0, (-ex).clamp(-120, 120), torch.zeros_like(ex)).long()


def _max_cols(M, NV):
    """column of each row's largest magnitude: the four waves (tid / 64), the first and the last register (c = tid + 256 k)"""
    cols = [0 + 256 * 0, (64 + 5) + 256 * (NV - 1), (128 + 9) + 256 * 0, (192 + 63) + 256 * (NV - 1), 70 + 256 * (NV // 2),
            200 + 256 * 1]
    return cols[:M]


def _scaled(v, f, dtype, sub=None, prev_exp=False, off_by_one=False, inv_as_scale=False, zero_inv=None):
    """rows of v (M, C) in dtype f times their power of two; sub: the columns the maximum is taken over"""
    mx = (v if sub is None else v[:, sub]).abs().amax(-1).double()
    e = row_exp(mx)
    if prev_exp:
        e = torch.roll(e, 1)
    if off_by_one:
        e = e + 1
    sc = torch.ldexp(torch.ones_like(mx), e)
    inv = sc.clone() if inv_as_scale else 1.0 / sc
    if zero_inv is not None:
        inv = torch.where(mx == 0, torch.full_like(inv, zero_inv), inv)
    return v * sc.to(f)[:, None], inv


def _assert_row_max(v64):
    mx = v64.abs().amax(-1)
    mant, _ = torch.frexp(mx[mx > 0])
    assert ((mant >= 0.55) & (mant <= 0.95)).all(), f"row maxima {mant.tolist()} outside [0.55, 0.95] x 2^m"


def scale_rows(C, with_gamma, dtype):
    """out (M, C) T = g * gamma * 2^e(row), inv[row] = 2^-e(row), M = 6: magnitudes 2^-100, 1e-6, 1 and 3e4, a zero row, and a row
    whose only non-zero is channel C - 1"""
    M, NV = 6, C // 256
    exps = [-100, -19, 0, 15, 0, -3]                                  # largest magnitudes 0.75 x 2^m
    cols = _max_cols(M, NV)
    cols[5] = C - 1
    gamma = signed((C,), 3, 0.25, 0.5) if with_gamma else None
    v = rnd((M, C), 1, 0.45).double()
    v = torch.where(v.abs() < 0.01, torch.full_like(v, 0.2), v)
    v[4], v[5] = 0.0, 0.0
    for r in range(M):
        if r != 4:
            v[r, cols[r]] = 0.75 * (-1.0) ** r
        v[r] *= 2.0 ** exps[r]
    g = (v / gamma.double()).float() if with_gamma else v.float()
    inp = {"g": g}
    if with_gamma:
        inp["gamma"] = gamma
    v64 = g.double() * (gamma.double() if with_gamma else 1.0)
    _assert_row_max(v64)
    assert (v64[4] == 0).all() and int((v64[5] != 0).sum()) == 1

    def closed(i, f, gamma_as=None, no_gamma=False, **kw):
        d = _f(i, f)
        gm = None if (no_gamma or "gamma" not in d) else (d["gamma"] if gamma_as is None else gamma_as.to(f))
        out, inv = _scaled(d["g"] * gm if gm is not None else d["g"], f, dtype, **kw)
        return {"out": out, "inv": inv}

    want = closed(inp, torch.float64)
    mk = lambda **kw: (lambda i: closed(i, torch.float64, **kw))
    defects = {"max_over_wave_0_only": mk(sub=[c for c in range(C) if c % 256 < 64]),
               "max_over_register_0_only": mk(sub=list(range(256))), "exponent_of_the_row_before": mk(prev_exp=True),
               "exponent_off_by_one": mk(off_by_one=True), "inv_is_2_to_e": mk(inv_as_scale=True),
               "zero_row_inv_not_1": mk(zero_inv=0.5)}
    if with_gamma:
        defects["gamma_omitted"] = mk(no_gamma=True)
        for name, gv in vec_variants(gamma).items():
            defects[f"gamma_{name}"] = mk(gamma_as=gv)
    kinds = {"out": ("T", want["out"] == 0), "inv": ("exact",)}
    case = _case("scale_rows", f"scale_rows C={C} gamma={'yes' if with_gamma else 'null'}", dtype, inp, want, kinds, closed,
                 defects)
    case.p = {"M": M, "C": C}
    return case


@torch.enable_grad()
def gelu_bwd(C4, dtype):
    """pre (M, 4C) T in place: pre <- dh * inv_in[row] * GELU'(pre) * 2^e(row), inv_out[row] = 2^-e(row); M = 5"""
    M, NV = 5, C4 // 256
    tmax = T_MAX[dtype]
    special = [0.0, 0.75, -0.75, 6.0, -6.0, 40.0, -40.0, tmax, -tmax]
    inv_in = torch.tensor([2.0 ** -3, 2.0 ** 5, 2.0 ** -20, 1.0, 2.0 ** 10])
    exps = [-7, 0, 3, -30, 12]
    cols = _max_cols(M, NV)
    pre = q(rnd((M, C4), 1, 2.0), dtype)
    pre[:, 10:10 + len(special)] = torch.tensor(special)
    gg = gelu_grad(pre.double())
    v = rnd((M, C4), 2, 0.4).double() * gg.abs().clamp(max=1.0)          # |v| <= 0.4 off the planted maximum
    dh = torch.empty((M, C4), dtype=torch.float64)
    for r in range(M):
        pre[r, cols[r]] = 0.75
        gg[r, cols[r]] = gelu_grad(torch.tensor(0.75, dtype=torch.float64))
        v[r, cols[r]] = 0.75 * (-1.0) ** r
        safe = torch.where(gg[r].abs() > 1e-3, gg[r], torch.ones_like(gg[r]))
        dh[r] = v[r] * 2.0 ** exps[r] / (inv_in[r].double() * safe)
    inp = {"dh": dh.float(), "inv_in": inv_in, "pre": pre}
    v64 = inp["dh"].double() * inv_in.double()[:, None] * gelu_grad(pre.double())
    _assert_row_max(v64)
    assert all((pre == sp).any() for sp in special)

    def closed(i, f, fwd=False, phi_only=False, neg=False, no_inv=False, inv_prev=False, dh_prev=False, **kw):
        d = _f(i, f)
        x = -d["pre"] if neg else d["pre"]
        gr = F.gelu(x) if fwd else gelu_grad(x, phi_only=phi_only)
        s = torch.ones_like(d["inv_in"]) if no_inv else (torch.roll(d["inv_in"], 1) if inv_prev else d["inv_in"])
        dhv = torch.roll(d["dh"], 1, 0) if dh_prev else d["dh"]
        out, inv = _scaled(dhv * s[:, None] * gr, f, dtype, **kw)
        return {"pre": out, "inv_out": inv}

    x = pre.double().requires_grad_(True)
    vg = torch.autograd.grad(F.gelu(x), x, inp["dh"].double() * inv_in.double()[:, None])[0]
    out, inv = _scaled(vg, torch.float64, dtype)
    want = {"pre": out, "inv_out": inv}
    mk = lambda **kw: (lambda i: closed(i, torch.float64, **kw))
    defects = {"gelu_for_its_derivative": mk(fwd=True), "phi_alone": mk(phi_only=True), "derivative_at_minus_x": mk(neg=True),
               "inv_in_omitted": mk(no_inv=True), "inv_in_of_the_row_before": mk(inv_prev=True),
               "dh_of_the_row_before": mk(dh_prev=True),
               "max_over_wave_0_only": mk(sub=[c for c in range(C4) if c % 256 < 64]),
               "max_over_register_0_only": mk(sub=list(range(256))), "exponent_of_the_row_before": mk(prev_exp=True),
               "exponent_off_by_one": mk(off_by_one=True), "inv_is_2_to_e": mk(inv_as_scale=True)}
    kinds = {"pre": ("T", None), "inv_out": ("exact",)}
    case = _case("gelu_bwd", f"gelu_bwd 4C={C4}", dtype, inp, want, kinds, closed, defects)
    case.p = {"M": M, "C": C4}
    return case


# ----------------------------------------------------------------------------- depthwise 7x7: LayerNorm backward, data gradient
def _taps(dw_w, C):
    """[49][C] -> (C, 1, 7, 7)"""
    return dw_w.reshape(7, 7, C).permute(2, 0, 1).unsqueeze(1)


def _dwconv(x, w4, b, clamp=False):
    """x (n, S, S, C) tokens -> raw depthwise output (n, S, S, C); clamp: edge replication where zeros belong"""
    C = x.shape[-1]
    xn = x.permute(0, 3, 1, 2)
    if clamp:
        y = F.conv2d(F.pad(xn, (3, 3, 3, 3), mode="replicate"), w4, b, groups=C)
    else:
        y = F.conv2d(xn, w4, b, padding=3, groups=C)
    return y.permute(0, 2, 3, 1)


@torch.enable_grad()
def dw_ln_bwd(C, side, nimg, dtype, small_var=False):
    """raw depthwise 7 x 7 output of a token with its LayerNorm statistics, then the LayerNorm backward over the row: ddw (rows, C).
    small_var: a constant bias, image 0 scaled down until a token's variance over the channels is of eps' size."""
    rows = nimg * side * side
    x = rnd((nimg, side, side, C), 1, 2.0)
    dw_b = torch.full((C,), 0.25) if small_var else signed((C,), 3, 0.25, 0.5)
    dw_w = signed((49, C), 2, 0.05, 0.15)
    if small_var:
        y0 = _dwconv(x[:1].double(), _taps(dw_w, C).double(), None)
        x[0] *= math.sqrt(EPS / y0[0, side // 2, side // 2].var(unbiased=False).item())
    inp = {"x": q(x, dtype), "dw_w": dw_w, "dw_b": dw_b, "ln_w": signed((C,), 4, 0.5, 1.0), "dxln": rnd((rows, C), 5, 0.9),
           "inv": 2.0 ** ((torch.arange(rows) * 7) % 23 - 11).float()}
    if small_var:
        var = _dwconv(inp["x"][:1].double(), _taps(dw_w, C).double(), dw_b.double())[0].var(-1, unbiased=False)
        assert ((var >= 0.3 * EPS) & (var <= 3 * EPS)).any(), f"no token of image 0 with a variance of eps' size: {var.flatten().tolist()}"

    def closed(i, f, ln_w=None, no_bias=False, tap_zeroed=False, flip=False, transpose=False, clamp=False, inv_prev=False,
               image_before=False, **ln):
        d = _f(i, f)
        w4 = _taps(d["dw_w"], C)
        if tap_zeroed:
            w4 = w4.clone()
            w4[C - 1, 0, 3, 3] = 0
        if flip:
            w4 = w4.flip(2, 3)
        if transpose:
            w4 = w4.transpose(2, 3)
        xs = _prev_last(d["x"]) if image_before else d["x"]
        y = _dwconv(xs, w4.contiguous(), None if no_bias else d["dw_b"], clamp).reshape(rows, C)
        inv = torch.roll(d["inv"], 1) if inv_prev else d["inv"]
        w = d["ln_w"] if ln_w is None else ln_w.to(f)
        return {"ddw": ln_bwd(y, d["dxln"] * inv[:, None] * w, EPS, **ln)}

    d = _f(inp, torch.float64)
    y = _dwconv(d["x"], _taps(d["dw_w"], C), d["dw_b"]).reshape(rows, C).detach().requires_grad_(True)
    z = F.layer_norm(y, (C,), d["ln_w"], None, EPS)
    want = {"ddw": torch.autograd.grad(z, y, d["dxln"] * d["inv"][:, None])[0]}
    s = want["ddw"].abs().amax(-1, keepdim=True)
    mk = lambda **kw: (lambda i: closed(i, torch.float64, **kw))
    defects = {"mean_dy_term_dropped": mk(no_mean=True), "projection_term_dropped": mk(no_proj=True),
               "rstd_omitted": mk(no_rstd=True), "ln_w_omitted": mk(ln_w=torch.ones(C)),
               "one_tap_zeroed_on_the_last_channel": mk(tap_zeroed=True)}
    for name, v in vec_variants(inp["ln_w"]).items():
        defects[f"ln_w_{name}"] = mk(ln_w=v)
    if small_var:
        defects["eps_omitted"] = mk(no_eps=True)
    else:
        defects["bias_omitted"] = mk(no_bias=True)
    if side > 1:
        defects.update({"taps_flipped": mk(flip=True), "ky_kx_transposed": mk(transpose=True),
                        "clamped_edge_for_zero_padding": mk(clamp=True)})
    if rows > 1:
        defects["inv_of_the_row_before"] = mk(inv_prev=True)
    if nimg > 1:
        defects["image_before"] = mk(image_before=True)
    case = _case("dw_ln_bwd", f"dw_ln_bwd C={C} side={side} n={nimg}" + (" small variance" if small_var else ""), dtype, inp,
                 want, {"ddw": ("scaled", s)}, closed, defects)
    case.p = {"C": C, "side": side, "nimg": nimg, "rows": rows}
    return case


@torch.enable_grad()
def dw_dgrad_res(C, side, nimg, dtype=F32):
    """g (rows, C) fp32 in place: g += depthwise 7 x 7 data gradient of ddw (flipped-tap correlation, zero padding, per image).
    No operand is in the storage dtype."""
    assert dtype == F32
    rows = nimg * side * side
    inp = {"ddw": rnd((rows, C), 1), "dw_w": signed((49, C), 2, 0.05, 0.15), "g": rnd((rows, C), 3, 0.5)}

    def closed(i, f, unflipped=False, res=1.0, clamp=False, tap_zeroed=False, transpose=False, image_before=False):
        d = _f(i, f)
        w4 = _taps(d["dw_w"], C)
        if tap_zeroed:
            w4 = w4.clone()
            w4[C - 1, 0, 3, 3] = 0
        if not unflipped:
            w4 = w4.flip(2, 3)
        if transpose:
            w4 = w4.transpose(2, 3)
        D = d["ddw"].reshape(nimg, side, side, C)
        if image_before:
            D = _prev_last(D)
        return {"g": res * d["g"] + _dwconv(D, w4.contiguous(), None, clamp).reshape(rows, C)}

    def grad(ddw, w):
        x = torch.zeros((nimg, C, side, side), dtype=torch.float64, requires_grad=True)
        y = F.conv2d(x, _taps(w, C), None, padding=3, groups=C)
        gx = torch.autograd.grad(y, x, ddw.reshape(nimg, side, side, C).permute(0, 3, 1, 2))[0]
        return gx.permute(0, 2, 3, 1).reshape(rows, C)

    d = _f(inp, torch.float64)
    want = {"g": d["g"] + grad(d["ddw"], d["dw_w"])}
    s = d["g"].abs() + grad(d["ddw"].abs(), d["dw_w"].abs())
    mk = lambda **kw: (lambda i: closed(i, torch.float64, **kw))
    defects = {"unflipped_taps": mk(unflipped=True), "residual_dropped": mk(res=0.0), "residual_added_twice": mk(res=2.0),
               "clamped_edge": mk(clamp=True), "one_tap_zeroed": mk(tap_zeroed=True), "ky_kx_transposed": mk(transpose=True)}
    if nimg > 1:
        defects["image_before"] = mk(image_before=True)
    case = _case("dw_dgrad_res", f"dw_dgrad_res C={C} side={side} n={nimg}", dtype, inp, want, {"g": ("scaled", s)}, closed,
                 defects)
    case.p = {"C": C, "side": side, "nimg": nimg, "rows": rows}
    return case


# ----------------------------------------------------------------------------- down_ln_bwd
@torch.enable_grad()
def down_ln_bwd(C2, side2, nimg, dtype):
    """depth-to-space of the patch gradient back to the stage-2 grid (an odd last row / column gets zero) + LayerNorm2d backward
    over C2: dA2 (nimg side2^2, C2).  Token 0 is scaled down to a variance of eps' size."""
    S, h2 = side2, side2 // 2
    rows2, rows3 = nimg * S * S, nimg * h2 * h2
    x = rnd((nimg, S, S, C2), 1, 2.0)
    x[0, 0, 0] *= 8.7e-4                                                # std 2 / sqrt 3 x that = 1e-3
    inp = {"x": q(x, dtype), "ln_w": signed((C2,), 4, 0.5, 1.0), "dP": rnd((rows3, 4 * C2), 5, 0.9),
           "inv": 2.0 ** ((torch.arange(rows3) * 5) % 19 - 9).float()}
    var = inp["x"][0, 0, 0].double().var(unbiased=False).item()
    assert 0.3 * EPS <= var <= 3 * EPS, f"variance of token 0: {var:.2e}"
    img, y, xx = torch.meshgrid(torch.arange(nimg), torch.arange(S), torch.arange(S), indexing="ij")
    live = ((y < 2 * h2) & (xx < 2 * h2)).reshape(-1)
    yy, xq = y.clamp(max=2 * h2 - 1), xx.clamp(max=2 * h2 - 1)

    def index(kx_ky=False, no_quadrant=False, side_for_h2=False, inv_by_tok=False, image_before=False):
        im = torch.where(img == nimg - 1, img - 1, img) if image_before else img
        row3 = im * h2 * h2 + (yy // 2) * (S if side_for_h2 else h2) + (xq // 2)
        quad = ((xq & 1) * 2 + (yy & 1)) if kx_ky else ((yy & 1) * 2 + (xq & 1))
        if no_quadrant:
            quad = torch.zeros_like(quad)
        row3 = row3.clamp(max=rows3 - 1).reshape(-1)
        irow = (torch.arange(rows2) % rows3) if inv_by_tok else row3
        return row3, quad.reshape(-1), irow

    def closed(i, f, ln_w=None, odd_left=False, idx=None, image_before=False, **ln):
        d = _f(i, f)
        row3, quad, irow = index(**(idx or {}), image_before=image_before)
        dP = d["dP"].reshape(rows3, 4, C2)[row3, quad] * d["inv"][irow][:, None]
        xs = d["x"]
        if image_before:
            xs = xs.clone()
            xs[nimg - 1] = xs[nimg - 2]
        w = d["ln_w"] if ln_w is None else ln_w.to(f)
        out = ln_bwd(xs.reshape(rows2, C2), dP * w, EPS, **ln)
        return {"dA2": torch.where(live[:, None], out, torch.full_like(out, SENT if odd_left else 0.0))}

    d = _f(inp, torch.float64)
    xg = d["x"].clone().requires_grad_(True)
    z = F.layer_norm(xg, (C2,), d["ln_w"], None, EPS)
    P = z[:, :2 * h2, :2 * h2].reshape(nimg, h2, 2, h2, 2, C2).permute(0, 1, 3, 2, 4, 5).reshape(rows3, 4 * C2)   # space-to-depth
    want = {"dA2": torch.autograd.grad(P, xg, d["dP"] * d["inv"][:, None])[0].reshape(rows2, C2)}
    s = want["dA2"].abs().amax(-1, keepdim=True)
    assert (s[~live] == 0).all() and (s[live] > 0).all()
    mk = lambda **kw: (lambda i: closed(i, torch.float64, **kw))
    defects = {"mean_dy_term_dropped": mk(no_mean=True), "projection_term_dropped": mk(no_proj=True),
               "rstd_omitted": mk(no_rstd=True), "eps_omitted": mk(no_eps=True), "ln_w_omitted": mk(ln_w=torch.ones(C2)),
               "quadrant_order_kx_ky": mk(idx={"kx_ky": True}), "quadrant_ignored": mk(idx={"no_quadrant": True})}
    for name, v in vec_variants(inp["ln_w"]).items():
        defects[f"ln_w_{name}"] = mk(ln_w=v)
    if S % 2:
        defects["odd_row_or_column_left_unwritten"] = mk(odd_left=True)
    base = index()
    for name, kw in (("row3_formed_with_side2_for_h2", {"side_for_h2": True}), ("inv_indexed_by_the_stage2_token", {"inv_by_tok": True})):
        alt = index(**kw)
        if any(not torch.equal(a[live], b[live]) for a, b in zip(alt, base)):      # the same index at this geometry: no defect
            defects[name] = mk(idx=kw)
    if nimg > 1:
        defects["image_before"] = mk(image_before=True)
    case = _case("down_ln_bwd", f"down_ln_bwd C2={C2} side2={side2} n={nimg}", dtype, inp, want, {"dA2": ("scaled", s)}, closed,
                 defects)
    case.p = {"C": C2, "side": side2, "nimg": nimg, "rows": rows2}
    return case


# ----------------------------------------------------------------------------- cam2
def cam2(C2, sides, B, dtype, up_pass=0, with224=True, gap=5):
    """alpha = spatial mean of d A2 per image, CAM = ReLU(sum_c alpha_c A2_c), optional 224 x 224 upsample of pass up_pass.
    `cam` is the whole (B, cam_ld) buffer with `gap` sentinel elements behind each map; alpha (npass, B, C2)."""
    hws = [s * s for s in sides]
    npass = len(sides)
    off = [sum(h + gap for h in hws[:p]) for p in range(npass)]
    cam_ld = off[-1] + hws[-1] + gap
    def make(attempt):
        inp = {}
        for p, hw in enumerate(hws):
            inp[f"A{p}"] = q(rnd((B, hw, C2), 10 + p + 100 * attempt, 2.0), dtype)
            inp[f"dA{p}"] = rnd((B, hw, C2), 20 + p + 100 * attempt)
        return inp

    inp = _search(make, lambda i: [(i[f"A{p}"].double() * i[f"dA{p}"].double().mean(1)[:, None, :]).sum(-1) for p in range(npass)],
                  f"cam2 C2={C2} sides={sides} B={B}")

    def closed(i, f, relu=True, half=True, swap=False, other_pass=False, drop_token=False, no_inv=False, image_before=False,
               passes_swapped=False, from_A=False, want_scale=False):
        d = _f(i, f)
        out = torch.full((B, cam_ld), 0.0 if want_scale else SENT, dtype=f)
        alphas, maps = [], []
        for p, hw in enumerate(hws):
            A, src = d[f"A{p}"], d[f"A{p}" if from_A else f"dA{p}"]
            if want_scale:
                A, src = A.abs(), src.abs()
            if image_before:
                A, src = _prev_last(A), _prev_last(src)
            al = (src[:, :hw - 1] if drop_token else src).sum(1) * (1.0 if no_inv else 1.0 / hw)
            pre = (A * al[:, None, :]).sum(-1)
            m = pre.clamp(min=0) if relu else pre
            out[:, off[p]:off[p] + hw] = m
            alphas.append(al)
            maps.append(m)
        if passes_swapped:
            alphas = alphas[::-1]
        res = {"cam": out, "alpha": torch.stack(alphas)}
        if with224:
            up = (1 - up_pass) if other_pass else up_pass
            res["cam224"] = upsample(maps[up].reshape(B, sides[up], sides[up]), half, swap)
        return res

    d = _f(inp, torch.float64)
    want = {"cam": torch.full((B, cam_ld), SENT, dtype=torch.float64), "alpha": torch.stack([d[f"dA{p}"].mean(1) for p in range(npass)])}
    for p, hw in enumerate(hws):
        pre = (d[f"A{p}"] * want["alpha"][p][:, None, :]).sum(-1)
        want["cam"][:, off[p]:off[p] + hw] = pre.clamp(min=0)
    sc = closed(inp, torch.float64, want_scale=True, relu=False)
    kinds = {"cam": ("scaled", sc["cam"]), "alpha": ("scaled", sc["alpha"])}
    if with224:
        S = sides[up_pass]
        m = want["cam"][:, off[up_pass]:off[up_pass] + S * S].reshape(B, 1, S, S)
        want["cam224"] = F.interpolate(m, size=(224, 224), mode="bilinear", align_corners=False)[:, 0]
        kinds["cam224"] = ("scaled", sc["cam224"])
    mk = lambda **kw: (lambda i: closed(i, torch.float64, **kw))
    defects = {"relu_omitted": mk(relu=False), "alpha_taken_from_A": mk(from_A=True)}
    if max(hws) > 1:
        defects["mean_over_hw_minus_1"] = mk(drop_token=True)
        defects["inv_hw_missing"] = mk(no_inv=True)
    if B > 1:
        defects["image_before"] = mk(image_before=True)
    if npass > 1:
        defects["passes_swapped"] = mk(passes_swapped=True)
    if with224:
        if sides[up_pass] > 1:
            defects["upsample_without_half_pixel_offset"] = mk(half=False)
            defects["upsample_x_y_swapped"] = mk(swap=True)
        if npass > 1:
            defects["upsample_of_the_other_pass"] = mk(other_pass=True)
    case = _case("cam2", f"cam2 C2={C2} sides={sides} B={B} up_pass={up_pass if with224 else None}", dtype, inp, want, kinds,
                 closed, defects)
    case.p = {"C": C2, "sides": sides, "hws": hws, "B": B, "up_pass": up_pass, "with224": with224, "off": off, "cam_ld": cam_ld}
    return case


# ----------------------------------------------------------------------------- the cases, shared by the CPU audit and the GPU tests
ALL = ("f32", "bf16", "f16")
CASES = [
    ("head-bwd-gelu-1x1-null", head_bwd, (1, 1, 2, None), ALL),                      # seven dead rows of the 8-row group
    ("head-bwd-gelu-8x8-ones", head_bwd, (8, 8, 2, "ones"), ALL),
    ("head-bwd-gelu-11x8-mixed", head_bwd, (11, 8, 2, "mixed"), ALL),                # a second group with a tail
    ("head-bwd-gelu-11x1-tie", lambda B, S, dt: head_bwd(B, S, 2, None, dt, tie=True), (11, 1), ALL),
    ("head-bwd-relu-11x8-tie-zeros", lambda B, S, dt: head_bwd(B, S, 1, None, dt, tie=True, zeros=True), (11, 8), ALL),
    ("head-bwd-relu-8x1-mixed", head_bwd, (8, 1, 1, "mixed"), ALL),
    ("bb-bwd-1x768", bb_bwd, (1, 768), ALL),
    ("bb-bwd-8x1536", bb_bwd, (8, 1536), ALL),
    ("bb-bwd-9x768", bb_bwd, (9, 768), ALL),
    ("bb-bwd-9x1536", bb_bwd, (9, 1536), ALL),
    ("pool-ln-bwd-768-49-9-tok0", lambda C, hws, B, dt: pool_ln_bwd(C, hws, B, dt, tok0=[0, 2 * 49 + 3]), (768, [49, 9], 2), ALL),
    ("pool-ln-bwd-1536-49-9", pool_ln_bwd, (1536, [49, 9], 1), ALL),
    ("pool-ln-bwd-768-one-token", pool_ln_bwd, (768, [1], 1), ALL),
    ("pool-ln-bwd-768-49-49", pool_ln_bwd, (768, [49, 49], 3), ALL),
    ("cam-768-7-3-up0", lambda C, sides, B, dt: cam(C, sides, B, dt, up_pass=0), (768, [7, 3], 2), ALL),
    ("cam-1536-7-3-up1", lambda C, sides, B, dt: cam(C, sides, B, dt, up_pass=1), (1536, [7, 3], 1), ALL),
    ("cam-768-one-token", lambda C, sides, B, dt: cam(C, sides, B, dt, up_pass=0), (768, [1], 1), ALL),
    ("cam-768-7-7-no-upsample", lambda C, sides, B, dt: cam(C, sides, B, dt, with224=False), (768, [7, 7], 3), ALL),
    ("scale-rows-768-gamma", scale_rows, (768, True), ALL),
    ("scale-rows-1536-gamma", scale_rows, (1536, True), ALL),
    ("scale-rows-768-null", scale_rows, (768, False), ALL),
    ("scale-rows-1536-null", scale_rows, (1536, False), ALL),
    ("gelu-bwd-3072", gelu_bwd, (3072,), ALL),
    ("gelu-bwd-6144", gelu_bwd, (6144,), ALL),
    ("dw-ln-bwd-768x1x2", dw_ln_bwd, (768, 1, 2), ALL),
    ("dw-ln-bwd-768x3x2", dw_ln_bwd, (768, 3, 2), ALL),
    ("dw-ln-bwd-768x7x1", dw_ln_bwd, (768, 7, 1), ALL),
    ("dw-ln-bwd-1536x5x2", dw_ln_bwd, (1536, 5, 2), ALL),
    ("dw-ln-bwd-768x3x2-small-variance", lambda C, s, n, dt: dw_ln_bwd(C, s, n, dt, small_var=True), (768, 3, 2), ALL),
    ("dw-dgrad-generic-100x2x2", dw_dgrad_res, (100, 2, 2), ("f32",)),
    ("dw-dgrad-generic-768x5x1", dw_dgrad_res, (768, 5, 1), ("f32",)),
    ("dw-dgrad-generic-300x7x2", dw_dgrad_res, (300, 7, 2), ("f32",)),
    ("dw-dgrad-img-768x7x2", dw_dgrad_res, (768, 7, 2), ("f32",)),
    ("dw-dgrad-img-1536x3x2", dw_dgrad_res, (1536, 3, 2), ("f32",)),
    ("dw-dgrad-img-256x3x1", dw_dgrad_res, (256, 3, 1), ("f32",)),
    ("down-ln-bwd-384x2x1", down_ln_bwd, (384, 2, 1), ALL),
    ("down-ln-bwd-384x3x2", down_ln_bwd, (384, 3, 2), ALL),                          # odd, h2 = 1
    ("down-ln-bwd-384x7x2", down_ln_bwd, (384, 7, 2), ALL),                          # the network's odd pass
    ("down-ln-bwd-768x14x1", down_ln_bwd, (768, 14, 1), ALL),
    ("cam2-384-14-7-up0", lambda C2, sides, B, dt: cam2(C2, sides, B, dt, up_pass=0), (384, [14, 7], 2), ALL),
    ("cam2-384-14-7-up1", lambda C2, sides, B, dt: cam2(C2, sides, B, dt, up_pass=1), (384, [14, 7], 2), ALL),
    ("cam2-768-3-no-upsample", lambda C2, sides, B, dt: cam2(C2, sides, B, dt, with224=False), (768, [3], 1), ALL),
    ("cam2-384-1-2-up1", lambda C2, sides, B, dt: cam2(C2, sides, B, dt, up_pass=1), (384, [1, 2], 2), ALL),
]
BY_NAME = {name: (build, args, dts) for name, build, args, dts in CASES}


def build(name, dtype):
    fn, args, _ = BY_NAME[name]
    return fn(*args, dtype)
