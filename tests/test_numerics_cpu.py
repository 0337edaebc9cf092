"""The bound functions of tests/test_numerics_gpu.py must be able to fail: each is run here, without a GPU, on a CPU
restatement of the device formula with one planted defect, and on the unmodified restatement, which must pass."""
import pytest
import torch

from tests import kcases, numutil as nu

torch.set_grad_enabled(False)

H16 = [torch.float16, torch.bfloat16]


def _value_sets(dtype):
    """the two 16-bit value sets of the GPU sweeps, as fp32 pre-activations: (name, pre, offgrid)"""
    grid = nu.shuffled(nu.finite_grid(dtype)).float()
    near = grid[grid.abs() <= 8]
    off = near + nu.tile_to(nu.offgrid_bias(96), near.numel())
    return [("on-grid", grid, False), ("off-grid", off, True)]


@pytest.mark.parametrize("dtype", H16, ids=["f16", "bf16"])
def test_gelu_restatement_passes_its_own_bound_and_delta_is_small(dtype):
    for name, pre, off in _value_sets(dtype):
        delta = nu.gelu_delta(pre, dtype, off)
        ok, ex = nu.gelu_h16_holds(nu.gelu_h16_ref(pre, dtype), pre, dtype, off, delta)
        print(f"{dtype} {name}: delta {delta:.3e} excess {ex:.3e}")
        assert ok
        # the polynomial's error beyond rounding is ~6e-4 (fit 1.1e-4 + the clamp's 1.3e-4 + fp16 Horner noise): a delta far
        # above that would make the GPU bound vacuous
        assert 0 < delta < 1e-3
        # the sites behind gelu_h16_n finish in fp32 for fp16 storage too; that form must sit inside the same delta
        ok, ex = nu.gelu_h16_holds(nu.gelu_h16_ref(pre, dtype, packed_finish=False), pre, dtype, off, delta)
        print(f"{dtype} {name}, fp32 finish: excess {ex:.3e}")
        assert ok


def _defects():
    c = list(nu.GELU_H16_COEF)
    c[3] += 1e-3
    return [("coefficient 3 off by 1e-3", dict(coef=tuple(c))), ("clamp at 3", dict(clamp=3.0)),
            ("pair swapped", dict(swap_pairs=True))]


@pytest.mark.parametrize("dtype", H16, ids=["f16", "bf16"])
@pytest.mark.parametrize("what,kw", _defects(), ids=["coef", "clamp3", "swap"])
def test_gelu_bound_rejects_a_defective_polynomial(dtype, what, kw):
    for name, pre, off in _value_sets(dtype):
        delta = nu.gelu_delta(pre, dtype, off)
        ok, ex = nu.gelu_h16_holds(nu.gelu_h16_ref(pre, dtype, **kw), pre, dtype, off, delta)
        print(f"{dtype} {name} {what}: delta {delta:.3e} excess {ex:.3e}")
        assert not ok, f"{what} passed the {name} bound: excess {ex:.3e} <= delta {delta:.3e}"


def test_gelu_f32_bound_rejects_the_16bit_polynomial():
    """the fp32 bound is relative to |x|: an absolute error of the 16-bit polynomial's size (6e-4) fails it near zero"""
    pre = nu.finite_grid(torch.float16).float()
    want = nu.gelu_ref(pre)
    assert ((want.float().double() - want).abs() <= nu.gelu_f32_bound(pre, want)).all()
    assert not ((nu.gelu_h16_ref(pre, torch.float16) - want).abs() <= nu.gelu_f32_bound(pre, want)).all()


@pytest.mark.parametrize("dtype", [torch.float32, torch.float16, torch.bfloat16], ids=["f32", "f16", "bf16"])
@pytest.mark.parametrize("C", [96, 384])
def test_layernorm_offset_bound_rejects_one_pass_statistics(dtype, C):
    w, b = nu.kutil.rnd((C,), 4, 0.5) + 1.0, nu.kutil.rnd((C,), 5, 0.1)
    for R in nu.OFFSETS:
        rows = nu.offset_rows(64, C, R)
        want = nu.ln_ref(rows, w, b, 1e-6)
        bound = nu.ln_offset_bound(dtype, R, nu.ln_torch_f32_err(rows, w, b, 1e-6, want))
        e2 = (nu.ln_twopass_ref(rows, w, b, 1e-6) - want).abs().max().item()
        e1 = (nu.ln_onepass_ref(rows, w, b, 1e-6) - want).abs().max().item()
        print(f"C={C} R={R}: bound {bound:.3e}  two-pass {e2:.3e}  one-pass {e1:.3e}")
        assert e2 <= bound, f"centred statistics must pass at R={R}"
        if R == 1000:
            assert not e1 <= bound, "one-pass statistics at |mean|/std = 1000 must fail"
    assert nu.mean_over_std(nu.offset_rows(64, C, 1000).double())[0] > 900


def test_layernorm_constant_bound_rejects_a_mean_of_16bit_precision():
    """constant rows of 100 (variance exactly 0, rstd = 1 / sqrt(eps) = 1000): the centred restatement passes (its mean is
    one ulp off at most: the sum is exact, 1 / C is not); a mean with a relative error of 2^-12, as a statistic kept in a
    16-bit type would have, is amplified to 37 and fails"""
    C, m = 96, 100.0
    w, b = nu.kutil.rnd((C,), 4, 0.5) + 1.0, nu.kutil.rnd((C,), 5, 0.1)
    rows = torch.full((4, C), m)
    for dtype in (torch.float32, torch.float16, torch.bfloat16):
        bound = nu.ln_const_bound(dtype, m, w.abs().max().item(), 1e-6)
        e2 = (nu.ln_twopass_ref(rows, w, b, 1e-6) - b.double()).abs().max().item()
        mean16 = rows.mean(-1, keepdim=True) * (1.0 + 2.0 ** -12)
        bad = (rows - mean16) * 1e3 * w + b
        e16 = (bad.double() - b.double()).abs().max().item()
        print(f"constant rows {dtype}: bound {bound:.3e}  centred {e2:.3e}  2^-12 mean {e16:.3e}")
        assert e2 <= bound and not e16 <= bound


# ----------------------------------------------------------------------------- softmax of the Swin window attention
_ATTN = (2, 14, 21, 96, 3, 3)
_UPPER = (torch.arange(49) & 4) != 0       # keys on the MFMA kernel's upper lane half


@pytest.mark.parametrize("dtype", [torch.float32, torch.float16, torch.bfloat16], ids=["f32", "f16", "bf16"])
@pytest.mark.parametrize("variant", ["uniform", "wide", "mask100"])
def test_softmax_cases_are_what_they_claim_and_reject_their_defects(variant, dtype):
    """The off-distribution softmax cases of tests/test_numerics_gpu.py (kcases.swin_attn's variants): the inputs have the
    property each case is named for, the honest float32 model passes the family's comparator, and every defect planted in
    the float64 restatement (the missing maximum in float32, where it overflows) is rejected by a factor 2."""
    case = kcases.swin_attn(*_ATTN, dtype, variant=variant)
    s = case.logits()
    if variant == "uniform":
        assert ((s == 0) | (s == -100)).all() and (s == -100).any()
    elif variant == "wide":
        span = s.amax(-1) - s.amin(-1)
        upper = _UPPER[s.argmax(-1)].double().mean().item()
        print(f"wide: logit span {span.min().item():.1f} .. {span.max().item():.1f}, largest logit {s.max().item():.1f}, "
              f"row maximum on the upper lane half in {upper:.2f} of the rows")
        assert span.min().item() >= 150 and 0.3 <= upper <= 0.7
        assert s.max().item() > 89, "exp of the largest logit must overflow fp32 for the missing maximum to show"
    else:
        plain = case.logits(mask=False)
        others = torch.arange(49) != 48
        lead = plain[..., 48] - plain[..., others].amax(-1)
        masked = (s[..., 48] < plain[..., 48] - 99)
        kept = s[..., 48] - s[..., others].amax(-1)
        print(f"mask100: key 48 leads by {lead.min().item():.1f} .. {lead.max().item():.1f} before the mask, by at least "
              f"{kept.min().item():.1f} after it; masked in {masked.double().mean().item():.2f} of the rows")
        assert 110 <= lead.min().item() and lead.max().item() <= 130 and kept.min().item() >= 10 and masked.any()
    want = case.want()
    m = case.measure(case.model(case.inputs), want)
    print(f"{case.what}: honest fp32 model err/bound {m['ratio']:.2f}, excess {m['excess']:.3e}")
    assert m["ratio"] <= 1.0
    for name, planted in case.defects.items():
        m = case.measure(case.to_storage(planted(case.inputs)), want)
        print(f"  {name:36s} max err {m['err']:.3e}  err/bound {m['ratio']:.1f}")
        assert m["ratio"] >= 2.0, f"{case.what}: {name} passes (err/bound {m['ratio']:.2f})"
