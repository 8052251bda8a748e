"""The Newton-statistics kernel (csrc/hip/glm.hip) against the float64 numpy reference
of test_glm.py, at the smallest shapes at which each part can go wrong, and
examples/LogisticRegression end to end on cuda:0."""
import pytest
import torch

from test_glm import normal, reference, run_job, small_ints, tens

pytestmark = pytest.mark.gpu

RUN = 4096
EXACT = [(0, 4, 1),             # an empty call
         (1, 1, 1),             # the smallest non-empty call
         (3, 5, 1),             # fewer rows than an MFMA step
         (70, 15, 1),           # p = 16, exactly one block
         (70, 16, 1),           # the ones column alone in a tail block
         (130, 60, 2),          # IL = 4 with the ones column inside a quad
         (130, 64, 2),          # NB = 5, IL = 1
         (300, 124, 1),         # NB = 8, IL = 4
         (300, 127, 1),         # the limit
         (2 * RUN + 7, 20, 1),  # widening
         (2 * RUN + 7, 20, 3)]  # uneven slabs


@pytest.mark.parametrize("n,d,slabs", EXACT)
def test_exact_at_beta_zero(gpu, n, d, slabs):
    from lua_mapreduce_1_amd.ops import glm as Gl
    X, y, beta = small_ints(n, d)
    t = tens(X, y, beta, device=gpu)
    reference(X, y, beta, Gl.newton_stats(*t, slabs=slabs), bounds=Gl.error_terms(*t, slabs), exact=True)


@pytest.mark.parametrize("n,d", [(4097, 15), (4097, 60), (9000, 127)])
def test_bounds_on_normal_points(gpu, n, d):
    from lua_mapreduce_1_amd.ops import glm as Gl
    X, y, beta = normal(n, d)
    t = tens(X, y, beta, device=gpu)
    for slabs in (1, 2):
        reference(X, y, beta, Gl.newton_stats(*t, slabs=slabs), bounds=Gl.error_terms(*t, slabs))


def test_running_state_and_reproducibility(gpu):
    from lua_mapreduce_1_amd.ops import glm as Gl
    tx, ty, tb = tens(*small_ints(5000, 33), device=gpu)
    whole = Gl.newton_stats(tx, ty, tb, slabs=2)
    acc = Gl.newton_stats(tx[:1234].contiguous(), ty[:1234].contiguous(), tb, slabs=1)
    got = Gl.newton_stats(tx[1234:].contiguous(), ty[1234:].contiguous(), tb, *acc, slabs=3)
    assert all(a is b for a, b in zip(got, acc))
    assert torch.equal(got[1], whole[1]) and torch.equal(got[2], whole[2])  # ll is not exact: log 2 per row
    t = tens(*normal(9000, 100), device=gpu)
    a, b = Gl.newton_stats(*t, slabs=5), Gl.newton_stats(*t, slabs=5)
    assert all(torch.equal(u, v) for u, v in zip(a, b))


def test_job_gpu_against_naive(gpu):
    from lua_mapreduce_1_amd.examples import LogisticRegression as m
    run_job(gpu, m.make_problem(5, 20_000, 16, 4), {"files": "synthetic", "n": 20_000, "nsplits": 4, "dim": 16, "seed": 5})
    assert m.BETA.is_cuda
