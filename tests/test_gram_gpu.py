"""The moments kernels (csrc/hip/gram.hip) against the float64 numpy reference of
test_gram.py, at the smallest shapes at which each part can go wrong, and
examples/PCA end to end on cuda:0."""
import pytest
import torch

from test_gram import normal, reference, run_job, small_ints, tens

pytestmark = pytest.mark.gpu

RUN = 4096
EXACT = [(0, 4, 0, 1, False),            # empty
         (1, 1, 0, 1, False),            # the smallest call
         (3, 5, 0, 1, False),            # fewer rows than an MFMA step, d % 4 != 0
         (70, 17, 0, 1, False),          # column tail, two blocks
         (130, 64, 1, 2, False),         # the 64-column group edge, a target
         (130, 65, 3, 2, False),         # an unaligned Y
         (300, 128, 0, 1, False),        # the last width whose waves split the rows (16-byte loads)
         (300, 129, 0, 1, False),        # the first whose waves split the blocks (4-byte fill)
         (200, 256, 0, 1, False),        # the limit (16-byte loads, interleaved blocks)
         (100, 192, 5, 1, True),         # 16-byte X chunk plus Y columns filled in place
         (2 * RUN + 7, 20, 0, 1, False),  # widening
         (2 * RUN + 7, 20, 0, 3, False),  # uneven slabs
         (2 * RUN + 7, 140, 0, 1, False),  # widening of the block-split kernel (runs of RUN / 2)
         (5000, 33, 2, 7, True)]         # a non-zero integer shift


@pytest.mark.parametrize("n,d,t,slabs,shift", EXACT)
def test_exact_on_small_integers(gpu, n, d, t, slabs, shift):
    from lua_mapreduce_1_amd.ops import gram as Gm
    X, Y, sh = small_ints(n, d, t, shift)
    reference(X, Y, sh, Gm.moments(*tens(X, Y, sh, device=gpu), slabs=slabs), exact=True)


@pytest.mark.parametrize("shift", [False, True])
@pytest.mark.parametrize("n,d,t", [(4097, 16, 0), (4097, 130, 3), (9000, 256, 0)])
def test_bounds_on_normal_points(gpu, n, d, t, shift):
    from lua_mapreduce_1_amd.ops import gram as Gm
    X, Y, sh = normal(n, d, t, shift)
    for slabs in (1, 2):
        reference(X, Y, sh, Gm.moments(*tens(X, Y, sh, device=gpu), slabs=slabs), factor=Gm.error_factor(n, slabs))


def test_running_state_and_reproducibility(gpu):
    from lua_mapreduce_1_amd.ops import gram as Gm
    X, Y, sh = small_ints(5000, 33, 2, True)
    tx, ty, ts = tens(X, Y, sh, device=gpu)
    whole = Gm.moments(tx, ty, ts, slabs=2)
    s, G = Gm.moments(tx[:1234].contiguous(), ty[:1234].contiguous(), ts, slabs=1)
    s2, G2 = Gm.moments(tx[1234:].contiguous(), ty[1234:].contiguous(), ts, s=s, G=G, slabs=3)
    assert s2 is s and G2 is G and torch.equal(s, whole[0]) and torch.equal(G, whole[1])
    tx, _ty, ts = tens(*normal(9000, 130, 0, True), device=gpu)
    a, b = Gm.moments(tx, None, ts, slabs=5), Gm.moments(tx, None, ts, slabs=5)
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])


def test_job_gpu_against_naive(gpu):
    from lua_mapreduce_1_amd.examples import KMeans as km
    m = run_job(gpu, km.make_points(5, 20_000, 16, 8, 4),
                {"files": "synthetic", "n": 20_000, "nsplits": 4, "dim": 16, "seed": 5}, 3)
    assert m.COMPONENTS.is_cuda and m.COVARIANCE.is_cuda and m.MEAN.is_cuda and m.EXPLAINED_VARIANCE.is_cuda
