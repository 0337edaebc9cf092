"""b2 of the narrow-stage fused ConvNeXt MLP kernels, made visible: a bias that is dropped, added twice, or handled once per
workgroup instead of once per token tile / pass must show.  So b2 is large here (|b2| in [2, 4], against 0.1 in the other
fused-MLP cases) and |gamma| is at least 0.05: a wrong bias moves an output by at least 0.05 * 2 = 0.1, far outside the
tolerances.  Inputs, float64 reference and the per-element comparator are those of the other fused-MLP cases
(tests/kcases.py, fused_mlp with b2_range = (2, 4): every other vector term stays away from zero as there, |gamma| >= 0.25),
the launches the ones of tests/test_kernels_gpu.py.  The kernels add b2 in the epilogue today; the cases are the ones a
kernel that starts GEMM2's accumulator at b2 has to pass as well.

Which kernel a shape reaches (cnx_mlp.h, fused_mlp.h): C = 96 runs fused_mlp_res_kernel from 65 536 tokens on and
fused_mlp_kernel<T, 96, 4> below; the LN-patchify epilogue exists at C = 96 only in the former (the entry refuses it below
65 536 tokens).  C = 192 always runs xs_mlp_kernel, on min(passes, 256) workgroups of one 256-token pass each, so a
workgroup sees a second pass from 65 537 tokens on.  The small shapes therefore check the bias on the first tile / pass,
ragged, and the shapes just above 65 536 tokens are the ones in which a wave runs a second tile (C = 96: 2 065 tiles on
2 048 waves) or a workgroup a second pass (C = 192: 258 passes on 256 workgroups; xs_mlp_kernel's accumulators start again
from the inline zero of the peeled first steps).  The small LN-patchify geometries (two images of 4 x 4 and of 6 x 6 tokens)
run alone at C = 192 and as the trailing segment behind 21 images of 56 x 56 at C = 96.  C = 384 runs the kernel pair
(xs_pw1 + pw2f), whose pw2f adds b2: 129 tokens are one ragged 128-token tile past the first, 1000 tokens several."""
import pytest
import torch

from tests.kutil import DTYPES
from tests.test_kernels_gpu import mlp_case, mlp_lnp_case

pytestmark = pytest.mark.gpu
torch.set_grad_enabled(False)

BIG_B2 = (2.0, 4.0)


@pytest.mark.parametrize("dt", ["bf16", "f16"])
@pytest.mark.parametrize("C,M", [
    (96, 33), (96, 8 * 32 * 2 + 1),        # one token past a 32-token tile; 513 tokens (fused_mlp_kernel<T, 96, 4>)
    (96, 65536 + 8 * 32 * 2 + 1),          # fused_mlp_res_kernel: 2 065 tiles on 2 048 waves, the last one ragged
    (192, 257), (192, 513),                # xs_mlp_kernel: 2 / 3 workgroups, ragged last pass
    (192, 65536 + 257),                    # 258 passes on 256 workgroups: second pass, the last one ragged
    (384, 129), (384, 1000),               # xs_pw1 + pw2f: ragged second 128-token tile; eight tiles, the last ragged
])
def test_bias_initialised_accumulator(dt, C, M):
    mlp_case(DTYPES[dt], C, M, b2_range=BIG_B2)


# segments: (images, H, W) per segment, in token order
_LNP = [
    (96, [(21, 56, 56), (2, 4, 4)]),       # 65 856 + 32 tokens: the two 4 x 4 images are one tile, some wave's second
    (96, [(21, 56, 56), (2, 6, 6)]),       # 65 856 + 72: two full tiles and a ragged one of 8 tokens
    (192, [(2, 4, 4)]),                    # 32 tokens
    (192, [(2, 6, 6)]),                    # 72 tokens
    (192, [(84, 28, 28), (2, 6, 6)]),      # 65 856 + 72: 258 passes on 256 workgroups, the second pass holds the 6 x 6 images
]


@pytest.mark.parametrize("dt", ["bf16", "f16"])
@pytest.mark.parametrize("C,segs", _LNP)
def test_bias_initialised_accumulator_layernorm_patchify(dt, C, segs):
    mlp_lnp_case(DTYPES[dt], C, segs, b2_range=BIG_B2)
