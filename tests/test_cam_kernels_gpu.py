"""The ten Grad-CAM backward kernels (csrc/cam.hip, csrc/cam_bwd.hip), one launch each through their gcv_k_* entry points, against
the autograd references of tests/camcases.py in f32, bf16 and f16 storage.  tests/test_kernel_sensitivity_cpu.py shows, without
a GPU, which planted defects these comparators reject.  Every output and in-place buffer lies inside a sentinel-filled
allocation with two guard rows in front and behind, asserted untouched; gaps inside an output (between the maps of a cam row,
between the passes of pool_ln_bwd) hold the sentinel in the reference too.  No case, row or element is skipped or filtered.
tests/test_cam_gpu.py and tests/test_cam2_gpu.py run the same kernels chained, on the networks."""
import pytest
import torch

from genconvit_amd import _lib
from tests import camcases, gemmcases, kcases, kutil
from tests.camcases import SENT
from tests.kutil import DTYPES, dev, gemm, ptr

pytestmark = pytest.mark.gpu

GUARD = 2
F32 = torch.float32
_KEEP = []


def D(t, dtype=None):
    """device copy that stays alive for the duration of the test"""
    if t is None:
        return None
    d = t.to(dev()) if dtype is None else t.to(dev(), dtype)
    _KEEP.append(d)
    if len(_KEEP) > 64:
        torch.cuda.synchronize()
        del _KEEP[:32]
    return d


class Guarded:
    """(rows, cols) of `dtype` between GUARD sentinel rows in front and behind; `init` is copied into the rows, else they hold the
    sentinel as well, so that an element the kernel never writes fails the comparison"""

    def __init__(self, rows, cols, dtype=F32, init=None):
        self.buf = torch.full((rows + 2 * GUARD, cols), SENT, dtype=dtype, device=dev())
        self.view = self.buf[GUARD:GUARD + rows]
        if init is not None:
            self.view.copy_(init.reshape(rows, cols).to(dev(), dtype))
        _KEEP.append(self.buf)

    def ptr(self):
        return self.view.data_ptr()

    def result(self, what):
        torch.cuda.synchronize()
        assert (self.buf[:GUARD].float() == SENT).all(), f"{what}: written in front of the buffer"
        assert (self.buf[GUARD + self.view.shape[0]:].float() == SENT).all(), f"{what}: written behind the buffer"
        return self.view


def _dt(dtype):
    return _lib.dtype_code(dtype)


def run_head_bwd(case, dtype):
    i, p = case.inputs, case.p
    out = Guarded(p["B"], 2000)
    kutil.call("gcv_k_head_bwd", _dt(dtype), ptr(D(i["partial"])), p["S"], ptr(D(i["b1"])), ptr(D(i["fc2_w"])),
               ptr(D(i["logits"])), ptr(D(i.get("target"))), ptr(D(i["fc_w"], dtype)), ptr(D(i["bb_pre"], dtype)), out.ptr(),
               p["B"], p["act"])
    return {"dfeat": out.result("dfeat")}


def run_bb_bwd(case, dtype):
    i, p = case.inputs, case.p
    out = Guarded(p["rows"], p["C"])
    kutil.call("gcv_k_bb_bwd", _dt(dtype), ptr(D(i["dfeat"])), ptr(D(i["W"], dtype)), out.ptr(), p["rows"], p["C"])
    return {"dpool": out.result("dpool")}


def _passes(i, key, dtype, n):
    return [D(i[f"{key}{q}"], dtype) if q < n else None for q in range(2)]


def _two(v):
    return list(v) + [0] * (2 - len(v))


def run_pool_ln_bwd(case, dtype):
    i, p = case.inputs, case.p
    A = _passes(i, "A", dtype, len(p["hws"]))
    out = Guarded(p["M"], p["C"])
    kutil.call("gcv_k_pool_ln_bwd", _dt(dtype), p["C"], len(p["hws"]), ptr(A[0]), ptr(A[1]), *_two(p["hws"]), *_two(p["tok0"]),
               ptr(D(i["lnw"])), ptr(D(i["dpool"])), out.ptr(), camcases.EPS, p["B"])
    return {"dA": out.result("dA")}


def _cam224(p):
    return Guarded(p["B"], 224 * 224) if p["with224"] else None


def run_cam(case, dtype):
    i, p = case.inputs, case.p
    A = _passes(i, "A", dtype, len(p["sides"]))
    out, up = Guarded(p["B"], p["cam_ld"]), _cam224(p)
    kutil.call("gcv_k_cam", _dt(dtype), p["C"], len(p["sides"]), ptr(A[0]), ptr(A[1]), *_two(p["sides"]), *_two(p["off"]),
               p["cam_ld"], p["up_pass"], ptr(D(i["lnw"])), ptr(D(i["dpool"])), out.ptr(), up.ptr() if up else None,
               camcases.EPS, p["B"])
    got = {"cam": out.result("cam")}
    if up:
        got["cam224"] = up.result("cam224").reshape(p["B"], 224, 224)
    return got


def run_scale_rows(case, dtype):
    i, p = case.inputs, case.p
    out, inv = Guarded(p["M"], p["C"], dtype), Guarded(p["M"], 1)
    kutil.call("gcv_k_scale_rows", _dt(dtype), ptr(D(i["g"])), ptr(D(i.get("gamma"))), out.ptr(), inv.ptr(), p["M"], p["C"])
    return {"out": out.result("out"), "inv": inv.result("inv").reshape(-1)}


def run_gelu_bwd(case, dtype):
    i, p = case.inputs, case.p
    pre, inv = Guarded(p["M"], p["C"], dtype, init=i["pre"]), Guarded(p["M"], 1)
    kutil.call("gcv_k_gelu_bwd", _dt(dtype), ptr(D(i["dh"])), ptr(D(i["inv_in"])), pre.ptr(), inv.ptr(), p["M"], p["C"])
    return {"pre": pre.result("pre"), "inv_out": inv.result("inv_out").reshape(-1)}


def run_dw_ln_bwd(case, dtype):
    i, p = case.inputs, case.p
    out = Guarded(p["rows"], p["C"])
    kutil.call("gcv_k_dw_ln_bwd", _dt(dtype), ptr(D(i["x"], dtype)), ptr(D(i["dw_w"])), ptr(D(i["dw_b"])), ptr(D(i["ln_w"])),
               ptr(D(i["dxln"])), ptr(D(i["inv"])), out.ptr(), p["nimg"], p["side"], p["C"], camcases.EPS)
    return {"ddw": out.result("ddw")}


def run_dw_dgrad_res(case, dtype=F32, channels=None):
    """channels: run on the first `channels` channels of the case's data, repacked to that width"""
    i, p = case.inputs, case.p
    C = channels or p["C"]
    g = Guarded(p["rows"], C, init=i["g"][:, :C].contiguous())
    kutil.call("gcv_k_dw_dgrad_res", ptr(D(i["ddw"][:, :C].contiguous())), ptr(D(i["dw_w"][:, :C].contiguous())), g.ptr(),
               p["nimg"], p["side"], C)
    return {"g": g.result("g")}


def run_down_ln_bwd(case, dtype):
    i, p = case.inputs, case.p
    out = Guarded(p["rows"], p["C"])
    kutil.call("gcv_k_down_ln_bwd", _dt(dtype), ptr(D(i["x"], dtype)), ptr(D(i["ln_w"])), ptr(D(i["dP"])), ptr(D(i["inv"])),
               out.ptr(), p["nimg"], p["side"], p["C"], camcases.EPS)
    return {"dA2": out.result("dA2")}


def run_cam2(case, dtype):
    i, p = case.inputs, case.p
    n = len(p["sides"])
    A, dA = _passes(i, "A", dtype, n), _passes(i, "dA", None, n)
    out, up, alpha = Guarded(p["B"], p["cam_ld"]), _cam224(p), Guarded(n * p["B"], p["C"])
    kutil.call("gcv_k_cam2", _dt(dtype), p["C"], n, ptr(A[0]), ptr(A[1]), ptr(dA[0]), ptr(dA[1]), *_two(p["sides"]),
               *_two(p["off"]), p["cam_ld"], p["up_pass"], out.ptr(), up.ptr() if up else None, alpha.ptr(), p["B"])
    got = {"cam": out.result("cam"), "alpha": alpha.result("alpha").reshape(n, p["B"], p["C"])}
    if up:
        got["cam224"] = up.result("cam224").reshape(p["B"], 224, 224)
    return got


RUN = {"head_bwd": run_head_bwd, "bb_bwd": run_bb_bwd, "pool_ln_bwd": run_pool_ln_bwd, "cam": run_cam,
       "scale_rows": run_scale_rows, "gelu_bwd": run_gelu_bwd, "dw_ln_bwd": run_dw_ln_bwd, "dw_dgrad_res": run_dw_dgrad_res,
       "down_ln_bwd": run_down_ln_bwd, "cam2": run_cam2}
_PARAMS = [pytest.param(name, dt, id=f"{name}-{dt}") for name, _, _, dts in camcases.CASES for dt in dts]


def _build(name, dt):
    return camcases.build(name, DTYPES[dt])


@pytest.mark.parametrize("name,dt", _PARAMS)
def test_cam_kernel_against_its_autograd_reference(name, dt):
    case = _build(name, dt)
    with torch.no_grad():
        got = RUN[case.family](case, DTYPES[dt])
        assert set(got) == set(case.parts)
        case.assert_close(got)


@pytest.mark.parametrize("dt", camcases.ALL)
def test_cam_is_the_relu_of_pool_ln_bwd_rows_dotted_with_the_tokens(dt):
    """cam_kernel forms g itself; pool_ln_bwd_kernel writes it to every token's row.  On the same inputs relu(row . A) and the map
    agree within the two kernels' own bounds: e_cam s_cam for the map, and e_pool s_pool sum_c |A_c| for the row's part."""
    dtype = DTYPES[dt]
    pool, cam = _build("pool-ln-bwd-768-49-9-tok0", dt), _build("cam-768-7-3-up0", dt)
    assert all(torch.equal(pool.inputs[k], cam.inputs[k]) for k in pool.inputs)
    with torch.no_grad():
        dA, maps = run_pool_ln_bwd(pool, dtype)["dA"].cpu().double(), run_cam(cam, dtype)["cam"].cpu().double()
        B = pool.p["B"]
        for q, hw in enumerate(pool.p["hws"]):
            A = pool.inputs[f"A{q}"].double()
            t0, off = pool.p["tok0"][q], cam.p["off"][q]
            rows = dA[t0:t0 + B * hw].reshape(B, hw, -1)
            s_pool = pool.scales["dA"][t0:t0 + B * hw].reshape(B, hw, -1)
            dot = (rows * A).sum(-1).clamp(min=0)
            bound = cam.parts["cam"].e * cam.scales["cam"][:, off:off + hw] + pool.parts["dA"].e * (s_pool * A.abs()).sum(-1)
            err = (dot - maps[:, off:off + hw]).abs()
            print(f"pass {q}: largest err / bound {(err / bound).max().item():.2f}")
            assert (err <= bound).all(), f"pass {q}: err / bound {(err / bound).max().item():.2f}"


@pytest.mark.parametrize("name", ["dw-dgrad-img-768x7x2", "dw-dgrad-img-1536x3x2"])
def test_dw_dgrad_per_image_kernel_sums_in_the_generic_kernels_order(name):
    """csrc/cam_bwd.hip says of dw_dgrad_res_img_kernel: "same summation order as the kernel above".  The generic kernel on the
    first 100 channels, repacked to C = 100, must return those channels of the per-image kernel's result bit for bit."""
    case = _build(name, "f32")
    assert case.p["C"] % 256 == 0 and case.p["side"] in (3, 7)              # launch_dw_dgrad_res' rule for the per-image kernel
    with torch.no_grad():
        img = run_dw_dgrad_res(case)["g"]
        generic = run_dw_dgrad_res(case, channels=100)["g"]
    case.assert_close({"g": img})
    assert torch.equal(generic, img[:, :100]), \
        f"largest difference {(generic - img[:, :100]).abs().max().item():.3e}"


@pytest.mark.parametrize("dt", camcases.ALL)
@pytest.mark.parametrize("N,K", gemmcases.cases(gemmcases.CAM_CONTRACTION))
def test_backward_contraction_gemm_with_one_split(dt, N, K):
    """The contractions between the backward kernels: launch_gemm with EPI_SPLITK, one split of the whole K, 13 rows"""
    dtype, M = DTYPES[dt], gemmcases.CAM_ROWS
    case = kcases.gemm("splitk", M, N, K, dtype, k_per_split=K)
    i = case.inputs
    part = Guarded(M, N)
    gemm(dtype, _lib.A_PLAIN, _lib.EPI_SPLITK, D(i["A"], dtype), D(i["W"], dtype), None, M, N, K, lda=K, partial=part.view,
         splitk=1, k_per_split=K)
    case.assert_close(part.result("partial"))


# ----------------------------------------------------------------------------- refusals
def _refused(name, *args):
    with pytest.raises(_lib.GenConViTHipError):
        kutil.call(name, *args)


def test_launchers_refuse_what_they_cannot_run():
    """C = 512, a map side of 8, side2 = 1, a null operand, an activation other than GELU / ReLU: an error from the launcher,
    nothing launched"""
    z = torch.zeros(1 << 20, device=dev())           # stands for every non-null operand: nothing reads it
    p, f32, e = z.data_ptr(), _dt(F32), camcases.EPS
    _refused("gcv_k_head_bwd", f32, p, 8, p, p, p, None, p, p, p, 2, _lib.ACT_LEAKY)
    _refused("gcv_k_head_bwd", f32, p, 8, p, p, p, None, p, p, None, 2, _lib.ACT_GELU)
    _refused("gcv_k_head_bwd", f32, p, 8, p, p, None, None, p, p, p, 2, _lib.ACT_GELU)        # neither logits nor target
    _refused("gcv_k_bb_bwd", f32, p, p, p, 2, 512)
    _refused("gcv_k_bb_bwd", f32, p, None, p, 2, 768)
    _refused("gcv_k_cam", f32, 512, 1, p, None, 7, 0, 0, 0, 49, 0, p, p, p, None, e, 1)
    _refused("gcv_k_cam", f32, 768, 1, p, None, 8, 0, 0, 0, 64, 0, p, p, p, None, e, 1)
    _refused("gcv_k_cam", f32, 768, 1, p, None, 7, 0, 0, 0, 49, 0, None, p, p, None, e, 1)
    _refused("gcv_k_cam", f32, 768, 2, p, None, 7, 3, 0, 49, 58, 0, p, p, p, None, e, 1)       # second pass without tokens
    _refused("gcv_k_pool_ln_bwd", f32, 512, 1, p, None, 49, 0, 0, 0, p, p, p, e, 1)
    _refused("gcv_k_pool_ln_bwd", f32, 768, 1, p, None, 49, 0, 0, 0, p, p, None, e, 1)
    _refused("gcv_k_scale_rows", f32, p, None, p, p, 2, 512)
    _refused("gcv_k_scale_rows", f32, p, None, None, p, 2, 768)
    _refused("gcv_k_gelu_bwd", f32, p, p, p, p, 2, 2048)
    _refused("gcv_k_gelu_bwd", f32, p, p, None, p, 2, 3072)
    _refused("gcv_k_dw_ln_bwd", f32, p, p, p, p, p, p, p, 1, 3, 512, e)
    _refused("gcv_k_dw_ln_bwd", f32, p, p, p, p, p, p, p, 1, 8, 768, e)
    _refused("gcv_k_dw_ln_bwd", f32, None, p, p, p, p, p, p, 1, 3, 768, e)
    _refused("gcv_k_dw_dgrad_res", p, p, p, 1, 8, 768)
    _refused("gcv_k_dw_dgrad_res", p, p, None, 1, 3, 768)
    _refused("gcv_k_down_ln_bwd", f32, p, p, p, p, p, 1, 2, 512, e)
    _refused("gcv_k_down_ln_bwd", f32, p, p, p, p, p, 1, 1, 384, e)
    _refused("gcv_k_down_ln_bwd", f32, p, p, None, p, p, 1, 2, 384, e)
    _refused("gcv_k_cam2", f32, 512, 1, p, None, p, None, 3, 0, 0, 0, 9, 0, p, None, p, 1)
    _refused("gcv_k_cam2", f32, 384, 1, p, None, p, None, 15, 0, 0, 0, 225, 0, p, None, p, 1)
    _refused("gcv_k_cam2", f32, 384, 1, p, None, p, None, 3, 0, 0, 0, 9, 0, p, None, None, 1)
    _refused("gcv_k_cam2", 7, 384, 1, p, None, p, None, 3, 0, 0, 0, 9, 0, p, None, p, 1)       # no such dtype
    torch.cuda.synchronize()
    assert (z == 0).all()
