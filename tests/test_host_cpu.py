"""CPU-only tests: the C-ABI library loads and exports every symbol include/genconvit_hip.h
declares, the host mirror keeps the reference's API surface / error behaviour, and the N>1 path
(frame shard -> all-gather -> reorder -> vote) is correct under gloo with world_size 2."""
import os
import re
import socket
import sys

import numpy as np
import pytest
import torch
import torch.multiprocessing as mp

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
torch.set_grad_enabled(False)


# ----------------------------------------------------------------------------- C ABI
def test_library_exports_every_declared_symbol():
    from genconvit_amd import _lib
    hdr = open(os.path.join(REPO, "include", "genconvit_hip.h")).read()
    declared = set(re.findall(r"\b(gcv_[a-z0-9_]+)\s*\(", hdr))
    assert declared, "no declarations parsed"
    lib = _lib.load()                       # raises if the .so is missing: no CPU fallback
    for name in sorted(declared):
        assert hasattr(lib, name), f"{name} declared in the header but not exported"
    assert declared == set(_lib.SIGNATURES), (declared ^ set(_lib.SIGNATURES))


def test_library_reads_two_environment_variables():
    """`strings libgenconvit_hip.so | grep ^GCV_` finds GCV_VAE_SPLIT and GCV_RCCL_PATH, nothing else.  A name
    the library hands to getenv is a string of its own, so an A/B switch that grows back shows here."""
    from genconvit_amd import _lib
    _lib.load()
    blob = open(_lib.LIB_PATH, "rb").read()
    runs = re.findall(rb"[\x20-\x7e\t]{4,}", blob)          # what strings(1) prints: printable runs of four or more
    assert len(runs) > 100, "no strings parsed"
    found = {r.decode() for r in runs if r.startswith(b"GCV_")}
    assert found == {"GCV_VAE_SPLIT", "GCV_RCCL_PATH"}, sorted(found)


def test_library_has_no_hard_hip_runtime_dependency():
    """The .so must bind to the process's HIP runtime (torch's bundled one), not bring a second."""
    import subprocess
    from genconvit_amd import _lib
    out = subprocess.run(["readelf", "-d", _lib.LIB_PATH], capture_output=True, text=True).stdout
    assert "amdhip64" not in out


def test_create_without_gpu_fails_loudly():
    if torch.cuda.is_available():
        pytest.skip("GPU present")
    import ctypes
    from genconvit_amd import _lib
    lib = _lib.load()
    h = ctypes.c_void_p()
    assert lib.gcv_create(ctypes.byref(h), 0, 0, 4) != 0
    assert "device" in _lib.last_error().lower()
    with pytest.raises(_lib.GenConViTHipError, match="no CPU fallback"):
        _lib.Handle(0, torch.float32, 4)


def test_product_never_imports_the_oracle():
    for root, _, files in os.walk(os.path.join(REPO, "genconvit_amd")):
        for f in files:
            if f.endswith(".py"):
                src = open(os.path.join(root, f)).read()
                assert not re.search(r"^\s*(from|import)\s+oracle\b", src, re.M), f"{f} imports the oracle"


DW_KINDS = ["tile", "tiny", "tiny_pair", "roll", "mfma", "pair"]    # gcv_dw_plan's kind codes (include/genconvit_hip.h)


def _dw_plan(dt, nimg, H, W, C, aligned=1):
    """gcv_dw_plan: (kind, grid, block, lds, band_rows) of a gcv_k_dwconv7_ln launch, or (rc, last error)."""
    import ctypes
    from genconvit_amd import _lib
    dtype = {"f32": torch.float32, "f16": torch.float16, "bf16": torch.bfloat16}[dt]
    out = (ctypes.c_int * 5)()
    rc = _lib.load().gcv_dw_plan(_lib.dtype_code(dtype), nimg, H, W, C, aligned, out)
    if rc:
        return rc, _lib.last_error()
    return (DW_KINDS[out[0]],) + tuple(out[1:])


def test_oracle_dispatch_thresholds_equal_the_product():
    """The same-dtype restatement rounds where the HIP path rounds, and two of those places depend on launch geometry:
    the C = 96 LayerNorm-patchify epilogue (fused_mlp_res_applies) and the matrix-pipe depthwise taps.  The oracle keeps
    its own constants; this asserts they are what the product computes."""
    from oracle import cpu_ref
    csrc = os.path.join(REPO, "genconvit_amd", "csrc")
    src = open(os.path.join(csrc, "fused_mlp.h")).read()
    m = re.search(r"fused_mlp_res_applies\(int C, int64_t M\)\s*\{\s*return C == 96 && M >= ([0-9 *]+);", src)
    assert m, "fused_mlp_res_applies changed shape: update the oracle's Launch rules with it"
    assert eval(m.group(1)) == cpu_ref.FUSED_LNP_MIN_TOKENS
    # the matrix-pipe dw kernel runs 16-bit C = 96 / 56-pixel-wide launches of DW_MFMA_MIN_IMAGE_ROWS image rows (images x H)
    # and more, and nothing else
    for nimg in range(1, 130):
        for H in (1, 28, 56, 57, 112):
            for dt in ("f16", "bf16"):
                want = nimg * H >= cpu_ref.DW_MFMA_MIN_IMAGE_ROWS
                assert (_dw_plan(dt, nimg, H, 56, 96)[0] == "mfma") == want, (dt, nimg, H)
            assert _dw_plan("f32", nimg, H, 56, 96)[0] != "mfma"
        for dt in ("f32", "f16", "bf16"):
            for C in (96, 192, 384, 768, 1536):
                for H in (1, 3, 7, 14, 28, 56):
                    if (C, H) != (96, 56):
                        assert _dw_plan(dt, nimg, H, H, C)[0] != "mfma", (dt, nimg, C, H)
    # and the rules as the restatement applies them: ED's two passes are one launch (B = 11 -> 68 992 tokens: fused, B = 10
    # -> 62 720: not), the matrix-pipe taps need 64 images of 56 rows in one dw launch
    la = cpu_ref.Launch(2 * 11 * 3136, 22)
    assert la.stage0_tokens >= cpu_ref.FUSED_LNP_MIN_TOKENS > 2 * 10 * 3136
    assert 63 * 56 < cpu_ref.DW_MFMA_MIN_IMAGE_ROWS <= 64 * 56


def test_dw_plan_table():
    """The depthwise 7x7 + LayerNorm launch, pinned: kernel kind, workgroups, threads, dynamic LDS bytes and rows per band
    of every dw launch of the ConvNeXt-T and ConvNeXt-L ED and VAE networks (both VAE schedules launch the same shapes) at
    B = 1 ... 256, of the GPU kernel tests, of unaligned operands and of the error cases, as recorded from the launcher
    before its choice moved into one plan (tests/golden/dw_plan.json)."""
    import json
    from tests import dwcases
    with open(os.path.join(REPO, "tests", "golden", "dw_plan.json")) as f:
        table = {tuple(r[:6]): r[6:] for r in json.load(f)["rows"]}
    need = set()
    for dt in ("f32", "f16", "bf16"):
        for widths in ((96, 192, 384, 768), (192, 384, 768, 1536)):
            for B in (1, 32, 33, 64, 67, 128, 256):
                for i, C in enumerate(widths):
                    need |= {(dt, 2 * B, 56 >> i, 56 >> i, C, 1),      # ED: both passes in one launch
                             (dt, B, 56 >> i, 56 >> i, C, 1),          # VAE: backbone(x), backbone(x_hat)
                             (dt, B, 28 >> i, 28 >> i, C, 1)}
        for C, H, W, n in dwcases.all_cases():       # the shapes the GPU parity tests run (tests/dwcases.py)
            need.add((dt, n, H, W, C, 1))
        need.add((dt, 2, 56, 56, 96, 0))              # ... and their unaligned 56 x 56 launch, which the launcher sends to Tile
    assert need <= set(table), sorted(need - set(table))[:5]
    kinds = {r[1] for r in table.values()}
    assert kinds == set(DW_KINDS) | {None}, kinds
    for key, (rc, *want) in table.items():
        got = _dw_plan(*key)
        if rc:
            assert got[0] == rc, (key, got)
            if rc == -3:
                assert "C must be one of" in got[1], got
        else:
            assert got == tuple(want), (key, got, want)


def test_every_dw_kernel_has_a_gpu_parity_case():
    """Per storage dtype, the kernels that gcv_dw_plan picks for the shapes of the GPU parity tests (tests/dwcases.py) are ALL
    the kernels dw_select (csrc/dwconv_impl.h) can return: as (kind, C, NS) for the band kernels, (kind, C, S) for the
    whole-map kernels, (tile, C, 0).  A kernel added to dw_select without a GPU case — or a case that stops reaching its
    kernel — fails here, without a GPU."""
    from tests import dwcases
    src = open(os.path.join(REPO, "genconvit_amd", "csrc", "dwconv_impl.h")).read()
    # the band kernels dw_select names, read from its source: the expected set above is the whole of them
    named = {(k.lower(), int(c), int(n)) for k, c, n in re.findall(r"go\(DwShape<DwKind::(Roll|Mfma|Pair), (\d+), (\d+)>\{\}\)", src)}
    assert named == dwcases.ROLL | dwcases.MFMA | dwcases.PAIR, named ^ (dwcases.ROLL | dwcases.MFMA | dwcases.PAIR)
    for dt in ("f32", "f16", "bf16"):
        got = set()
        for C, H, W, n in dwcases.all_cases():
            plan = _dw_plan(dt, n, H, W, C)
            assert isinstance(plan[0], str), (dt, C, H, W, n, plan)
            kind = plan[0]
            got.add((kind, C, W // 7 if kind in ("roll", "mfma", "pair") else H if kind in ("tiny", "tiny_pair") else 0))
        assert got == dwcases.reachable(dt), (dt, sorted(got ^ dwcases.reachable(dt)))
        # the unaligned launch of the GPU tests is the tile kernel's
        assert _dw_plan(dt, 2, 56, 56, 96, aligned=0)[0] == "tile"
    # the intent of each list: what it was written to reach
    for dt in ("f32", "f16", "bf16"):
        for C, H, W, n in dwcases.TILE + dwcases.TILE_ODD:
            assert _dw_plan(dt, n, H, W, C)[0] == "tile", (dt, C, H, W, n)
        for C, H, W, n in dwcases.TILE_ODD:
            assert (n * -(-H // 7) * -(-W // 7)) % 2 == 1
            assert _dw_plan(dt, n, H, W, C)[1] == (n * -(-H // 7) * -(-W // 7) + 1) // 2
        kinds = {_dw_plan(dt, n, H, W, C)[0] for C, H, W, n in dwcases.BANDS}
        assert kinds == ({"roll", "pair"} if dt == "f32" else {"roll", "pair", "mfma"}), (dt, kinds)


def test_every_launch_geometry_the_networks_reach_has_a_kernel_case():
    """The pattern of the test above, applied to geometry.  tests/census.py walks, through the library's planners, every
    depthwise and MLP launch of ED, VAE (both schedules) and gcv_convnext_forward at every accepted resolution on both
    backbones at B = 1 ... the handle limit; the geometry keys it reaches must EQUAL the keys that the explicit case lists
    cover (tests/dwcases.py GEOMETRY and MERGED, tests/kcases.py PAIR384_M + PAIR384_SPLIT_M + PAIR384_TILE_M and PERSISTENT).  A geometry
    without a case fails; a case that stops reaching its geometry fails; and since every entry is the only one with its key
    in some storage dtype, so does a list with one entry removed."""
    from tests import census, dwcases, kcases
    tiny, large = census.reached("tiny"), census.reached("large")
    for dt, dtype in census.DTYPES.items():
        # depthwise band kernels: (kind, C, NS, H, band_rows), each entry at the smallest image count that reaches its key
        want = dict(large["dw"][dt])
        for key, n in tiny["dw"][dt].items():
            want[key] = min(n, want.get(key, n))
        have = {}
        for C, H, plan in dwcases.GEOMETRY:
            key = census.dw_key(dt, plan, H, C)
            assert key not in have, (dt, "two GEOMETRY entries with one key", key, have[key], plan)
            have[key] = plan
        assert have == want, (dt, sorted(set(have.items()) ^ set(want.items())))
        assert set(dwcases.GEOMETRY_N3) <= set(dwcases.GEOMETRY)
        n3 = {census.dw_key(dt, plan, H, C)[:3] for C, H, plan in dwcases.GEOMETRY_N3}
        assert n3 == {k[:3] for k in want}, (dt, "three images once per band kernel", n3)
        # what the GPU test builds for an entry is what the census keyed
        for C, H, plan in dwcases.GEOMETRY:
            assert kcases.dw_plan(dtype, plan, H, H, C) == (census.dw_key(dt, plan, H, C)[0], census.dw_key(dt, plan, H, C)[4])
        # merged launches: the pair of keys; ConvNeXt-L has none
        assert not large["dw2"][dt]
        have2 = {}
        for C, H0, H1, p0, p1 in dwcases.MERGED:
            assert census.dw_merged(dt, p0, H0, p1, H1, C), (dt, C, H0, H1, p0, p1)
            key = (census.dw_key(dt, p0, H0, C), census.dw_key(dt, p1, H1, C))
            assert key not in have2, (dt, "two MERGED entries with one pair of keys", key)
            have2[key] = (p0, p1)
        assert have2 == tiny["dw2"][dt], (dt, sorted(set(have2.items()) ^ set(tiny["dw2"][dt].items())))
        if dt == "f32":
            assert not tiny["mlp"][dt] and not large["mlp"][dt]      # two tile GEMMs: tests/gemmcases.py
            continue
        reached = set(tiny["mlp"][dt]) | set(large["mlp"][dt])
        # C = 384: (hidden-range split ns, pw2 tile)
        new_m = kcases.PAIR384_SPLIT_M + kcases.PAIR384_TILE_M
        plans = {M: kcases.mlp_plan(dtype, 384, M) for M in kcases.PAIR384_M + new_m}
        key = lambda M: (plans[M][2], plans[M][4:7])
        assert {k[1:] for k in reached if k[0] == "pair384"} == {key(M) for M in plans}, \
            (dt, {k[1:] for k in reached if k[0] == "pair384"} ^ {key(M) for M in plans})
        assert {p[2]: p[3] for p in plans.values()} == {ns: 48 // ns for ns in (1, 2, 3, 4, 6, 8, 12, 24)}
        assert {plans[M][2] for M in kcases.PAIR384_M} == {1, 3, 8, 24}
        assert [plans[M][2] for M in kcases.PAIR384_SPLIT_M] == [12, 6, 4, 2]
        # each new case is the only one with its key, at the smallest token count that has it, one token into its last tile
        old = {key(M) for M in kcases.PAIR384_M}
        for M in new_m:
            assert key(M) not in old and [m for m in new_m if key(m) == key(M)] == [M], (M, key(M))
            first = next(m for m in range(1, M + 1, 256) if (lambda p: (p[2], p[4:7]))(kcases.mlp_plan(dtype, 384, m)) == key(M))
            assert first == M, (M, first)
            assert kcases.xs_pw1_range(384, M) == 32 * 48 // plans[M][2]
        # persistent kernels: (kernel, epilogue, passes as 1 / 2 / 3 and more)
        keys = [kcases.persistent_key(dtype, *entry) for entry in kcases.PERSISTENT]
        assert len(set(keys)) == len(keys), (dt, "two PERSISTENT entries with one key", keys)
        assert set(keys) == {k for k in reached if k[0] != "pair384"}, (dt, set(keys) ^ {k for k in reached if k[0] != "pair384"})
        # the plan of a capped launch: the cap bounds the grid, the passes follow
        assert kcases.mlp_plan(dtype, 192, 2352, 3)[1:4] == (10, 3, 4) and kcases.mlp_plan(dtype, 192, 2352)[1:4] == (10, 10, 1)
        assert kcases.mlp_plan(dtype, 96, 70013, 64)[1:5] == (1, 64, 2188, 5) and kcases.mlp_plan(dtype, 96, 70013)[1:5] == (1, 256, 2188, 2)
        assert kcases.mlp_plan(dtype, 96, 65535)[1:5] == (0, 512, 2048, 1)
    import ctypes
    from genconvit_amd import _lib
    out = (ctypes.c_int * 8)()
    assert _lib.load().gcv_mlp_plan(_lib.GCV_F16, 192, 2352, 0, out) != 0 and "workgroup cap" in _lib.last_error()
    assert _lib.load().gcv_mlp_plan(_lib.GCV_F16, 192, 2352, 257, out) != 0


def test_gemm_plan_table():
    """The GEMM family's launch, pinned: kernel (tile GEMM and its tile, LDS-DMA GEMM and its LDS row, direct conv), grid,
    threads and dynamic LDS bytes of every launch_gemm call of the ED and VAE networks on both backbones (both VAE schedules),
    their explain passes and Swin-T at B = 1 ... 256 (tests/gemmcases.py has the formulas), of every GPU GEMM test, of the
    operand alignments that change the kernel and of every error.  tests/golden/gemm_plan.json was recorded from the
    launchers as they were before the choice moved into gemm_select: in a copy of that source, outside the repository, the
    three functions that launched (launch_cfg, launch_glds_bkb, launch_conv_direct_cfg) wrote their template parameters,
    grid, block and LDS bytes into a thread-local and returned, and gcv_k_gemm was called on the CPU for every row."""
    import json
    from tests import gemmcases as gc
    with open(os.path.join(REPO, "tests", "golden", "gemm_plan.json")) as f:
        gold = json.load(f)
    assert gold["columns"] == list(gc.Launch._fields) + ["f32", "f16_bf16"]
    assert gold["plan"] == ["kernel", "grid_x", "grid_y", "threads", "lds"]
    table = {gc.Launch(*r[:-2]): r[-2:] for r in gold["rows"]}
    assert gc.table_launches() <= set(table), sorted(gc.table_launches() - set(table))[:5]
    text = dict(gc.ERRORS)
    for l, per_dt in table.items():
        for dt, want in zip(("f32", "f16", "bf16"), per_dt + per_dt[1:]):
            got = gc.plan(dt, l)
            if isinstance(want, int):
                assert got[0] == want, (dt, l, got)
                assert l not in text or text[l] in got[1], (dt, l, got)
            else:
                assert got == tuple(gold["kernels"][want[0]]) + tuple(want[1:]), (dt, l, got, want)
    for l, msg in gc.ERRORS:
        assert all(isinstance(v, int) for v in table[l]), (l, msg)


def _gemm_kernels_named(dt):
    """the (kind, five tile fields, a_mode, epi) that gemm_select (csrc/gemm_impl.h) names for storage dtype dt, read from
    its source: go(Route{}, Shape<...>{}) calls, the conv tiles once per route they are called with"""
    from genconvit_amd import _lib
    csrc = os.path.join(REPO, "genconvit_amd", "csrc")
    src = open(os.path.join(csrc, "gemm_impl.h")).read()
    body = src[src.index("int gemm_select("):src.index("int gemm_plan(")]
    routes = {name: (getattr(_lib, a), getattr(_lib, e))
              for a, e, name in re.findall(r"typedef Route<(A_\w+), (EPI_\w+)[^>]*> (\w+);", src)}
    calls = re.findall(r"\bgo\((\w+)(?:\{\})?, (Tile|Glds|Direct)Shape<([^>]*)>\{\}\)", body)
    assert len(calls) == body.count("Shape<") == 26, (len(calls), body.count("Shape<"))
    conv_routes = re.findall(r"\btiles\((\w+)\{\}\)", body)
    assert sorted(conv_routes) == ["ConvPool", "ConvS2"]
    built = int(re.search(r"#define GCV_CONV_DIRECT (\d+)", open(os.path.join(csrc, "conv_direct.h")).read()).group(1))
    named = set()
    for route, kind, targs in calls:
        v = [(64 if dt == "f32" else 128) if t == "B" else int(t) for t in targs.split(", ")]
        if kind == "Tile":
            for r in (conv_routes if route == "route" else [route]):
                named.add(("tile", *v) + routes[r])
        elif dt != "f32" and kind == "Glds":
            named.add(("glds", 128, 192, 64, 96, v[0]) + routes[route])
        elif dt != "f32" and (built >> ((0 if v[1] == 1 else 2) + (v[0] == 32))) & 1:      # conv_direct_on
            named.add(("direct", v[0], v[1], 0, 0, 0) + routes[route])
    return named


def test_gemm_case_lists_reach_the_kernels_they_state():
    """tests/gemmcases.py states, next to every case of the GPU GEMM tests, the kernel it was written for; gcv_gemm_plan must
    agree for the launch as the test makes it (shape, leading dimensions, operand alignment)."""
    from tests import gemmcases as gc
    for dt in ("f32", "f16", "bf16"):
        for l, kernel in gc.gpu_launches(dt):
            assert gc.plan(dt, l)[:6] == gc.resolve(kernel, dt), (dt, l, gc.plan(dt, l))
    # and the alignment rules: the launch next to each aligned one leaves the LDS-DMA / direct kernel in 16-bit storage
    kinds = [gc.plan("f16", l)[0] for l in gc.ALIGNMENT]
    assert kinds == ["glds", "tile", "tile", "glds", "tile", "tile", "direct", "tile", "tile", "direct", "direct", "tile"], kinds


def test_every_gemm_kernel_has_a_gpu_parity_case():
    """Per storage dtype, the kernels that gcv_gemm_plan picks for the launches of the GPU parity tests (tests/gemmcases.py)
    are ALL the kernels gemm_select (csrc/gemm_impl.h) names, as (kind, tile, a_mode, epilogue); one activation per kernel
    is enough.  A kernel added to gemm_select without a GPU case — or a case that stops reaching its kernel — fails here,
    without a GPU."""
    from tests import gemmcases as gc
    for dt in ("f32", "f16", "bf16"):
        named = _gemm_kernels_named(dt)
        assert len(named) == (17 if dt == "f32" else 30), (dt, len(named))
        got = {gc.plan(dt, l)[:6] + (l.a_mode, l.epi) for l, _ in gc.gpu_launches(dt)}
        assert got == named, (dt, sorted(got ^ named, key=str))


_ARCH_DIMS = {0: (96, 192, 384, 768), 1: (192, 384, 768, 1536)}      # GCV_CONVNEXT_TINY / _LARGE (csrc/net.h)


def test_every_accepted_resolution_has_a_dw_plan_at_every_stage():
    """gcv_convnext_forward takes res = 32 ... 224 in steps of 4.  The four maps of a pass are res / 4 pixels wide, halved
    with floor at each stage boundary; gcv_dw_plan must have a kernel for each of them at any batch (16-byte aligned: the
    pass's token buffers are 256-byte aligned arena blocks, and a segment starts a whole number of C-channel tokens in) — or
    gcv_convnext_res_ok, the rule convnext_forward itself applies before it launches anything, refuses the resolution.
    Both directions: a resolution with all four plans is not refused."""
    from genconvit_amd import _lib
    lib = _lib.load()
    refused = {0: [], 1: []}
    for arch, dims in _ARCH_DIMS.items():
        for res in range(32, 228, 4):
            w, planned = res // 4, True
            for C in dims:
                for dt in ("f32", "f16", "bf16"):
                    for B in (1, 3, 256):
                        planned = planned and isinstance(_dw_plan(dt, B, w, w, C)[0], str)
                w //= 2
            ok = lib.gcv_convnext_res_ok(arch, res) == 1
            assert ok == planned, (arch, res, ok, planned)
            if not ok:
                refused[arch].append(res)
    assert refused[0] == [] and refused[1] == list(range(160, 224, 4)), refused
    for arch in (0, 1):
        for res in (0, 28, 30, 33, 34, 226, 228, 448, -32):
            assert lib.gcv_convnext_res_ok(arch, res) == 0, (arch, res)


def test_isa_report_checks_on_synthetic_assembly(tmp_path):
    """csrc/isa_report.py runs on every build; its three checks on small hand-written listings: the wide-store hazard,
    an inline-asm load whose register is touched before the asm s_waitcnt — also when the load sits at the END of a loop body
    and the touch at its head (the back-edge pass) — and the scratch budget."""
    import importlib.util
    spec_ = importlib.util.spec_from_file_location("isa_report", os.path.join(REPO, "genconvit_amd", "csrc", "isa_report.py"))
    isa = importlib.util.module_from_spec(spec_)
    spec_.loader.exec_module(isa)

    def listing(body, scratch=0):
        return ("_Z4testv:\n" + body + "\ts_endpgm\n.Lfunc_end0:\n"
                "  - .agpr_count:     0\n    .group_segment_fixed_size: 0\n    .name:           _Z4testv\n"
                f"    .private_segment_fixed_size: {scratch}\n    .sgpr_count:     10\n    .vgpr_count:     8\n"
                "    .vgpr_spill_count: 0\n")

    def findings(body, scratch=0):
        f = tmp_path / "k.s"
        f.write_text(listing(body, scratch))
        return isa.check_file(str(f)) + isa.check_scratch(str(f))

    clean = ("\t;;#ASMSTART\n\tglobal_load_dwordx4 v[4:7], v[0:1], off\n\t;;#ASMEND\n"
             "\t;;#ASMSTART\n\ts_waitcnt vmcnt(0)\n\t;;#ASMEND\n\tv_add_f32 v1, v5, v5\n")
    assert findings(clean) == []
    early = ("\t;;#ASMSTART\n\tglobal_load_dwordx4 v[4:7], v[0:1], off\n\t;;#ASMEND\n\tv_add_f32 v1, v5, v5\n")
    assert len(findings(early)) == 1 and "check 2" in findings(early)[0]
    loop = (".LBB0_1:\n\tv_add_f32 v1, v5, v5\n\t;;#ASMSTART\n\ts_waitcnt vmcnt(0)\n\t;;#ASMEND\n\tv_mov_b32 v2, v5\n"
            "\t;;#ASMSTART\n\tglobal_load_dwordx4 v[4:7], v[0:1], off\n\t;;#ASMEND\n\ts_cbranch_scc1 .LBB0_1\n")
    got = findings(loop)
    assert len(got) == 1 and "back-edge" in got[0], got
    loop_ok = loop.replace(".LBB0_1:\n\tv_add_f32 v1, v5, v5\n", ".LBB0_1:\n\tv_add_f32 v1, v3, v3\n")
    assert findings(loop_ok) == []
    store = "\tbuffer_store_dwordx4 v[10:13], v2, s[4:7], s2 offen\n\tv_mov_b32 v10, v3\n"
    assert len(findings(store)) == 1 and "check 1" in findings(store)[0]
    assert len(findings(clean, scratch=64)) == 1 and "check 3" in findings(clean, scratch=64)[0]


# ----------------------------------------------------------------------------- host mirror API
def test_config_keys():
    from genconvit_amd.model.config import load_config
    c = load_config()
    assert c["model"]["backbone"] == "convnext_tiny"
    assert c["model"]["embedder"] == "swin_tiny_patch4_window7_224"
    assert c["model"]["latent_dims"] == 12544 and c["img_size"] == 224 and c["num_classes"] == 2


def test_state_dict_keys_match_reference_layout():
    from genconvit_amd.model.config import load_config
    from genconvit_amd.model.genconvit_ed import GenConViTED
    m = GenConViTED(load_config(), init="empty")
    keys = set(m.state_dict())
    for k in ("encoder.features.0.weight", "encoder.features.12.bias", "decoder.features.8.weight",
              "backbone.stem.0.weight", "backbone.stem.1.bias", "backbone.stages.1.downsample.1.weight",
              "backbone.stages.2.blocks.8.mlp.fc2.weight", "backbone.stages.3.blocks.2.gamma",
              "backbone.head.norm.weight", "backbone.head.fc.bias", "fc.weight", "fc2.bias"):
        assert k in keys, k
    assert m.state_dict()["backbone.stages.0.blocks.0.conv_dw.weight"].shape == (96, 1, 7, 7)
    assert m.state_dict()["fc.weight"].shape == (500, 2000) and m.num_features == 2000
    # published checkpoints also carry the never-executed Swin embedder twice: accepted and ignored
    sd = dict(m.state_dict())
    sd["embedder.layers.0.blocks.0.attn.qkv.weight"] = torch.zeros(288, 96)
    sd["backbone.patch_embed.proj.weight"] = torch.zeros(768, 1000, 1, 1)
    m.load_state_dict(sd)                   # strict=True must not complain about those
    sd.pop("fc.weight")
    with pytest.raises(RuntimeError, match="fc.weight"):
        m.load_state_dict(sd)


def test_forward_on_cpu_raises_instead_of_falling_back():
    from genconvit_amd import _lib
    from genconvit_amd.model.config import load_config
    from genconvit_amd.model.genconvit_ed import GenConViTED
    m = GenConViTED(load_config(), init="empty")
    assert next(m.parameters()).device.type == "cpu"          # pred_vid's device discovery works
    if not torch.cuda.is_available():
        with pytest.raises(_lib.GenConViTHipError, match="no CPU fallback"):
            m(torch.zeros(1, 3, 224, 224))


def test_missing_weight_file_error_text(tmp_path, monkeypatch):
    from genconvit_amd.model.config import load_config
    from genconvit_amd.model.genconvit import GenConViT
    monkeypatch.chdir(tmp_path)
    with pytest.raises(Exception, match=r"Error: weight/nope_ed.pth file not found."):
        GenConViT(load_config(), ed="nope_ed", vae="nope_vae", net="ed", fp16=False)
    with pytest.raises(Exception, match=r"Error: weight/nope_vae.pth file not found."):
        GenConViT(load_config(), ed="nope_ed", vae="nope_vae", net="vae", fp16=False)
    with pytest.raises(Exception, match=r"Error: Model weights file not found."):
        GenConViT(load_config(), ed="nope_ed", vae="nope_vae", net="genconvit", fp16=False)


def test_checkpoint_layouts_load(tmp_path, monkeypatch):
    """raw state_dict and {'state_dict': ...} layouts of weight/{name}.pth (model/genconvit.py:16-21)."""
    from genconvit_amd import spec, synth
    from genconvit_amd.model.config import load_config
    from genconvit_amd.model.genconvit import GenConViT
    monkeypatch.chdir(tmp_path)
    os.mkdir("weight")
    sd = synth.make_state_dict(spec.ed_spec(), 7, "ed/")
    torch.save(sd, "weight/raw_ed.pth")
    torch.save({"epoch": 3, "state_dict": sd}, "weight/wrapped_ed.pth")
    for name in ("raw_ed", "wrapped_ed"):
        g = GenConViT(load_config(), ed=name, vae="unused", net="ed", fp16=False)
        assert torch.equal(g.model_ed.state_dict()["fc2.weight"], sd["fc2.weight"])
        assert not g.model_ed.training          # sub-network .eval() as model/genconvit.py:23
    g = GenConViT(load_config(), ed="raw_ed", vae="unused", net="ed", fp16=True)
    assert next(g.parameters()).dtype == torch.float16


def test_pred_func_surface():
    import genconvit_amd.model.pred_func as pf
    for name in ("load_genconvit", "face_rec", "preprocess_frame", "pred_vid", "max_prediction_value", "real_or_fake",
                 "extract_frames", "df_face", "is_video", "set_result", "store_result", "torch", "os", "np"):
        assert hasattr(pf, name), name            # prediction.py star-imports these (prediction.py:6,253)
    assert pf.real_or_fake(0) == "FAKE" and pf.real_or_fake(1) == "REAL"
    y = torch.tensor([[0.9, 0.2], [0.7, 0.4]])
    assert pf.max_prediction_value(y) == (0, pytest.approx(0.8))
    y = torch.tensor([[0.1, 0.8], [0.3, 0.6]])
    idx, val = pf.max_prediction_value(y)
    assert idx == 1 and val == pytest.approx(abs(1 - 0.7))
    r = pf.store_result(pf.set_result(), "a.mp4", 1, 0.3, "Fake", "FAKE")
    assert r["video"] == {"name": ["a.mp4"], "pred": [0.3], "klass": ["fake"], "pred_label": ["REAL"],
                          "correct_label": ["FAKE"]}
    assert not pf.is_video("/nonexistent.mp4")


def test_preprocess_frame_matches_oracle():
    import genconvit_amd.model.pred_func as pf
    from genconvit_amd import synth
    from oracle import cpu_ref
    u8 = synth.make_uint8_frames(3).numpy()
    got = pf.preprocess_frame(u8).cpu()
    want = cpu_ref.preprocess_frame(u8)
    assert got.shape == (3, 3, 224, 224) and torch.allclose(got, want, atol=1e-6)
    assert torch.equal(synth.make_frames(3), want)


def test_hybrid_embed_probe():
    """model/model_embedder.py:16-37 with a (1,1000)-logit backbone: grid (1,1000), proj 1000->768,
    and forward raises for 2-D logits exactly like the reference."""
    from genconvit_amd.model.model_embedder import HybridEmbed

    class Logits(torch.nn.Module):
        def __init__(self):
            super().__init__()
            self.w = torch.nn.Parameter(torch.zeros(1))

        def forward(self, x):
            return torch.zeros(x.shape[0], 1000)
    he = HybridEmbed(Logits(), img_size=224, embed_dim=768)
    assert he.grid_size == (1, 1000) and tuple(he.proj.weight.shape) == (768, 1000, 1, 1)
    with pytest.raises(RuntimeError):
        he(torch.zeros(2, 3, 224, 224))


# ----------------------------------------------------------------------------- N>1 path under gloo
def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _worker(rank, world, port, n_frames, nets, q):
    import torch.distributed as dist
    sys.path.insert(0, REPO)
    from genconvit_amd import dist as gdist
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    g = torch.Generator().manual_seed(5)
    frames = torch.rand((n_frames, 3, 4, 4), generator=g)

    def fake_forward(x, eps):          # stand-in per-frame "network": rows [ed; vae] of the shard
        f = x.flatten(1)
        ed = torch.stack([f.sum(1), f.mean(1)], 1)
        return ed if nets == 1 else torch.cat([ed, torch.stack([f.max(1).values, f.min(1).values], 1)], 0)
    full = gdist.sharded_forward(fake_forward, frames, None, nets)
    want = fake_forward(frames, None)
    q.put((rank, torch.equal(full, want), tuple(full.shape)))
    dist.destroy_process_group()


@pytest.mark.parametrize("n_frames,nets", [(8, 2), (7, 2), (1, 2), (5, 1)])
def test_sharded_gather_equals_unsharded_gloo_world2(n_frames, nets):
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=_worker, args=(r, 2, port, n_frames, nets, q)) for r in range(2)]
    for p in procs:
        p.start()
    res = [q.get(timeout=120) for _ in procs]
    for p in procs:
        p.join(timeout=60)
        assert p.exitcode == 0
    for rank, ok, shape in res:
        assert ok, f"rank {rank} reassembled tensor differs"
        assert shape == (nets * n_frames, 2)


def test_shard_bounds_cover_and_balance():
    from genconvit_amd.dist import shard_bounds
    for n in (0, 1, 7, 8, 128, 1024, 1023):
        for w in (1, 2, 3, 8):
            b = [shard_bounds(n, w, r) for r in range(w)]
            assert b[0][0] == 0 and b[-1][1] == n
            assert all(b[i][1] == b[i + 1][0] for i in range(w - 1))
            sizes = [hi - lo for lo, hi in b]
            assert max(sizes) - min(sizes) <= 1


# ----------------------------------------------------------------------------- drop-in claim: the upstream driver's surface
def test_prediction_driver_surface_on_the_model_alias(tmp_path, monkeypatch):
    """alias ``model`` -> ``genconvit_amd.model`` in sys.modules and run the two imports the
    upstream ``prediction.py`` starts with (``from model.pred_func import *``, ``from model.config import load_config``),
    then make the calls its ``vids()`` / ``predict()`` make, in the same order and with the same arguments: load_config,
    set_result, load_genconvit from a cwd-relative ``weight/`` file, is_video, pred_vid (forward stubbed: no GPU here),
    store_result, real_or_fake, and the (0, 0.5) default for a video without faces.  Checks the star-import surface
    (``torch`` / ``os`` reach the driver through it) and the ``store_result`` schema that ends up in result/*.json."""
    import json
    import genconvit_amd.model as gm
    from genconvit_amd import spec, synth
    names = ("config", "genconvit", "genconvit_ed", "genconvit_vae", "model_embedder", "pred_func")
    saved = {k: sys.modules.get(k) for k in ["model"] + [f"model.{n}" for n in names]}
    try:
        sys.modules["model"] = gm
        for n in names:
            sys.modules[f"model.{n}"] = __import__(f"genconvit_amd.model.{n}", fromlist=["_"])
        monkeypatch.chdir(tmp_path)                      # weight/, model/config.yaml and result/ are cwd-relative
        (tmp_path / "weight").mkdir()
        (tmp_path / "vids").mkdir()
        torch.save({"state_dict": synth.make_state_dict(spec.ed_spec(), 7, "ed/")}, tmp_path / "weight" / "ed_w.pth")
        for n in ("a.mp4", "b.avi", "notes.txt"):
            (tmp_path / "vids" / n).write_bytes(b"0")
        pred = {}
        exec("from model.pred_func import *\nfrom model.config import load_config\n", pred)
        for name in ("load_genconvit", "df_face", "pred_vid", "is_video", "set_result", "store_result", "real_or_fake",
                     "load_config", "torch", "os"):
            assert name in pred, f"the star import did not provide `{name}`"
        config = pred["load_config"]()
        assert config["model"]["backbone"] == "convnext_tiny"

        def fake_forward(self, x, eps=None):             # stands in for the HIP forward (no GPU in this container)
            return torch.tensor([[2.0, -1.0]] * x.shape[0])

        from genconvit_amd.model.genconvit import GenConViT
        monkeypatch.setattr(GenConViT, "forward", fake_forward)
        result = pred["set_result"]()
        model = pred["load_genconvit"](config, "ed", "ed_w", "unused_vae", False)
        assert isinstance(model, GenConViT) and not model.training
        vids = sorted(os.listdir(tmp_path / "vids"))
        assert [pred["is_video"](os.path.join(tmp_path, "vids", v)) for v in vids] == [True, True, False]
        for v in vids[:2]:
            df = synth.make_frames(3, name=v)
            y, y_val = pred["pred_vid"](df, model)
            result = pred["store_result"](result, v, y, y_val, "uncategorized", "unknown", None)
        v = result["video"]
        assert set(v) == {"name", "pred", "klass", "pred_label", "correct_label"}
        assert v["name"] == ["a.mp4", "b.avi"]
        assert v["klass"] == ["uncategorized"] * 2 and v["correct_label"] == ["unknown"] * 2
        assert v["pred_label"] == ["FAKE", "FAKE"]                       # index 0 = FAKE (pred_func.py:134-135)
        assert all(abs(p - float(torch.sigmoid(torch.tensor(2.0)))) < 1e-6 for p in v["pred"])
        json.dumps(result)                                               # what main() writes to result/*.json
        # a video without faces: predict() stores (0, 0.5) without calling the model
        y, y_val = torch.tensor(0).item(), torch.tensor(0.5).item()
        r2 = pred["store_result"](pred["set_result"](), "x.mp4", y, y_val, "uncategorized", "unknown", None)
        assert r2["video"]["pred_label"] == ["FAKE"] and pred["real_or_fake"](y) == "FAKE"
    finally:
        for k, m in saved.items():
            if m is None:
                sys.modules.pop(k, None)
            else:
                sys.modules[k] = m


# ----------------------------------------------------------------------------- row N2: host-resident big parameters
def test_big_parameters_stay_on_the_host_and_follow_the_dtype():
    """The VAE's 25088x12544 Linear weights (1.26 GB each in fp32) must not be moved to the device as nn.Parameters:
    `.half()` / `.to(dtype)` change their dtype, `.to(device)` leaves them where they are; every other parameter follows
    `_apply` as usual and state_dict() keeps the reference's keys."""
    from genconvit_amd.model import _base
    from genconvit_amd.model.config import load_config
    from genconvit_amd.model.genconvit_vae import GenConViTVAE
    m = GenConViTVAE(load_config(), init="empty")
    big = [n for n, p in m.named_parameters() if p.numel() >= _base.HOST_RESIDENT_NUMEL]
    assert sorted(big) == ["encoder.fc1.weight", "encoder.mu.weight", "encoder.var.weight"] or "encoder.mu.weight" in big
    m.half()
    sd = m.state_dict()
    assert sd["encoder.mu.weight"].dtype == torch.float16 and sd["encoder.mu.weight"].device.type == "cpu"
    assert sd["fc.weight"].dtype == torch.float16
    assert sd["encoder.mu.weight"].shape == (12544, 25088)
    dev, dt = m._param_device_dtype()          # device discovery ignores the host-resident tensors
    assert dt == torch.float16 and dev.type == "cpu"
    assert m._chunks(1100) == [(0, 512), (512, 1024), (1024, 1100)]


def test_same_dtype_restatement_is_the_identity_in_fp32_and_close_in_16_bit():
    """oracle/cpu_ref.py::storage_dtype — fp32 must leave the pinned oracle bit-for-bit unchanged; fp16 / bf16 round at
    the HIP path's storage points and stay within the deltas the MI355X shows (tests/test_parity_gpu.py gates on both)."""
    from genconvit_amd import spec, synth
    from oracle import cpu_ref
    sd = synth.make_state_dict(spec.ed_spec(), synth.DEFAULT_SEED, "ed/")
    x = synth.make_frames(1)
    base = cpu_ref.ed_forward(sd, x)
    with cpu_ref.storage_dtype(torch.float32):
        assert torch.equal(cpu_ref.ed_forward(sd, x), base)
    with cpu_ref.storage_dtype(torch.float16):
        d16 = (cpu_ref.ed_forward(sd, x) - base).abs().max().item()
    with cpu_ref.storage_dtype(torch.bfloat16):
        db = (cpu_ref.ed_forward(sd, x) - base).abs().max().item()
    assert cpu_ref._STORE is None                # the context restores the default
    assert 0 < d16 < 2e-3 and d16 < db < 3e-2, (d16, db)


def test_gelu_polynomial_in_the_kernels_is_what_the_fit_produces():
    """The coefficients of GeluH16 (genconvit_amd/csrc/gemm.h: the 16-bit paths' GELU on the packed-fp16 pipe) are the
    degree-8 fit on [0, 4] of profiles/gelu_fit.py times -1/2, and that fit, evaluated the way the instruction sequence
    evaluates it (numpy model of fp16 fma chains), keeps the stored fp16 activation within the error quoted in DESIGN.md
    section 4.0 item 7.  timm ConvNeXtBlock's exact GELU is the reference."""
    import re, sys
    import numpy as np
    from numpy.polynomial import chebyshev as Ch
    from scipy.special import erf
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    sys.path.insert(0, os.path.join(root, "profiles"))
    import gelu_fit
    src = open(os.path.join(root, "genconvit_amd", "csrc", "gemm.h")).read()
    body = src[src.index("struct GeluH16 {"):]
    assert "static constexpr int DEG = 8;" in body
    m = re.search(r"kC\[DEG \+ 1\] = \{(.*?)\};", body, re.S)
    kc = [eval(t.replace("f", "").strip()) for t in m.group(1).split(",")]
    err, co = gelu_fit.fit(4.0, 8, iters=600)
    mono = Ch.cheb2poly(co)
    assert err < 1.2e-4 and len(kc) == 9
    assert np.abs(np.array(kc) + 0.5 * mono).max() < 2e-6          # the polynomial carries -h/2
    assert "(u16x2){0x4400, 0x4400}" in body and "k2(0.5f), k2(-1.0f)" in body     # clamp 4.0, t = a/2 - 1
    # numpy model of the sequence with the committed coefficients: fp32 tail (bf16 storage) and packed tail (fp16 storage)
    f16 = np.float16
    fma = lambda a, b, c: (a.astype(np.float64) * b.astype(np.float64) + c.astype(np.float64)).astype(f16)
    x = (np.random.default_rng(0).standard_normal(400_000) * 1.5).astype(np.float32)
    xh = x.astype(f16)
    a = np.minimum(np.abs(xh), f16(4.0))
    t = fma(a, np.full_like(a, f16(0.5)), np.full_like(a, f16(-1)))
    c16 = [f16(v) for v in kc]
    p = fma(np.full_like(t, c16[8]), t, np.full_like(t, c16[7]))
    for k in range(6, -1, -1):
        p = fma(p, t, np.full_like(t, c16[k]))
    truth = 0.5 * x.astype(np.float64) * (1 + erf(x.astype(np.float64) / np.sqrt(2)))
    y32 = (np.maximum(x, 0).astype(np.float64) + 2 * p.astype(np.float64)).astype(np.float32).astype(f16)
    ypk = fma(p, np.full_like(p, f16(2)), np.maximum(xh, f16(0)))
    rms = lambda y: float(np.sqrt(((y.astype(np.float64) - truth) ** 2).mean()))
    exact = rms(truth.astype(np.float32).astype(f16))
    assert exact < 2.2e-4 and rms(y32) < 2.6e-4 and rms(ypk) < 3.5e-4


# ----------------------------------------------------------------------------- the stage-by-stage tap check catches tile bugs
@pytest.mark.parametrize("dtype", ["float16", "bfloat16"])
@pytest.mark.parametrize("stage,block,seg,tok", [(0, 1, 0, 0), (0, 2, 1, 1000), (2, 4, 1, 10)])
def test_tap_check_catches_a_skipped_tile(stage, block, seg, tok, dtype, monkeypatch):
    """The check of tests/test_taps_gpu.py, with its committed bounds, on the same-dtype oracle against the same oracle in
    which one 32-token tile of image 0 of one backbone segment skips one ConvNeXt block (its output = its input): the first
    tap out of bounds is that block's output, at that tile.  The unmodified oracle passes."""
    import torch
    from genconvit_amd import synth
    from oracle import cpu_ref
    from tests import taputil
    from tests.conftest import synthetic_sd
    torch.set_grad_enabled(False)
    sd, x, dtype = synthetic_sd("ed"), synth.make_frames(2), getattr(torch, dtype)
    lay, bounds = taputil.layout("ed", 2), taputil.BOUNDS[dtype]

    def oracle():
        taps = {}
        with cpu_ref.storage_dtype(dtype):
            cpu_ref.ed_forward(sd, x, taps)
        return taps

    clean = oracle()
    assert not taputil.failures(taputil.compare(clean, oracle(), lay, bounds))

    orig, calls = cpu_ref.convnext_block, []
    target = f"backbone.stages.{stage}.blocks.{block}."

    def skipping(sd_, p, xin, store=True, mfma_taps=False):
        y = orig(sd_, p, xin, store=store, mfma_taps=mfma_taps)
        if p == target:
            calls.append(p)
            if len(calls) == seg + 1:      # segment order of the ED token stream: [recon, orig]
                y = y.clone()
                c = y.shape[1]
                y[0].view(c, -1)[:, tok:tok + 32] = xin[0].reshape(c, -1)[:, tok:tok + 32]
        return y

    monkeypatch.setattr(cpu_ref, "convnext_block", skipping)
    bad = taputil.failures(taputil.compare(oracle(), clean, lay, bounds))
    assert bad, "a skipped tile went unnoticed"
    first = bad[0]
    assert first["name"] == f"ed.bb.s{stage}.b{block}", first["where"]
    assert (first["seg"], first["img"]) == (taputil.BB_SEGMENTS["ed"][seg][0], 0), first["where"]
    assert tok <= first["tok"] < tok + 32, first["where"]
    print(f"\n{dtype} skip of stage {stage} block {block}: {first['where']} (bound {first['bound']})")
