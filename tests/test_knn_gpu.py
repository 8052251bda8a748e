"""The k-nearest-neighbour kernels (csrc/hip/knn.hip) against the float64 numpy
reference of test_knn.py, at the smallest shapes at which each part can go
wrong, and examples/KNN end to end on cuda:0."""
import numpy as np
import pytest
import torch

from test_knn import normal, reference, run_job, small_ints, tens

pytestmark = pytest.mark.gpu

EXACT = [(1, 1, 1, 1, 1, "rand"),           # the smallest call
         (17, 5, 3, 64, 1, "rand"),         # n < K: padding with inf / -1
         (65, 64, 129, 16, 1, "rand"),      # tails: two query blocks, two tiles
         (1000, 130, 65, 32, 3, "rand"),    # d not a multiple of 4, d-chunks, uneven slabs
         (300, 512, 17, 64, 2, "rand"),     # d at the limit
         (100003, 8, 5, 64, 1, "rand"),     # many tiles, many compactions
         (100003, 8, 5, 64, 7, "rand"),
         (5000, 16, 257, 64, 1, "sorted"),  # descending distance to query 0: every tile passes the threshold
         (5000, 16, 257, 64, 1, "same"),    # all rows identical: the lowest indices win
         (0, 4, 9, 3, 1, "rand")]           # empty X


@pytest.mark.parametrize("n,d,q,k,slabs,kind", EXACT)
def test_exact_on_small_integers(gpu, n, d, q, k, slabs, kind):
    from lua_mapreduce_1_amd.ops import knn as N
    Q, X = small_ints(n, d, q, kind)
    reference(Q, X, k, N.search(*tens(Q, X, device=gpu), k, slabs=slabs), exact=True)


@pytest.mark.parametrize("n,d,q,k", [(200, 5, 130, 16), (1000, 130, 65, 32), (5000, 16, 257, 64), (4097, 64, 200, 33)])
def test_bounds_on_normal_points(gpu, n, d, q, k):
    from lua_mapreduce_1_amd.ops import knn as N
    Q, X = normal(n, d, q)
    reference(Q, X, k, N.search(*tens(Q, X, device=gpu), k), min_clear=0.85)


def test_piecewise_equals_whole(gpu):
    from lua_mapreduce_1_amd.ops import knn as N
    k, base = 33, 2 ** 33 + 5
    tq, tx = tens(*normal(4097, 64, 200), device=gpu)
    whole = N.search(tq, tx, k, base=base)
    got = [N.search(tq, tx, k, base=base, slabs=s) for s in (1, 4)]
    dist = idx = None
    for lo, hi in ((0, 70), (70, 3001), (3001, 4097)):
        dist, idx = N.search(tq, tx[lo:hi].contiguous(), k, dist, idx, base=base + lo)
    got.append((dist, idx))
    got.append(N.merge(*N.search(tq, tx[:1500].contiguous(), k, base=base),
                       *N.search(tq, tx[1500:].contiguous(), k, base=base + 1500)))
    for g in got:
        assert torch.equal(g[0], whole[0]) and torch.equal(g[1], whole[1])
    assert int(whole[1].min()) >= base and int(whole[1].max()) < base + 4097


def test_job_gpu_against_naive(gpu):
    from lua_mapreduce_1_amd.examples import KMeans as km
    queries = np.random.default_rng(1).normal(0, 10, (300, 16)).astype(np.float32)
    m = run_job(gpu, km.make_points(5, 20_000, 16, 8, 4),
                {"files": "synthetic", "n": 20_000, "nsplits": 4, "dim": 16, "seed": 5}, queries, 10)
    assert m.DISTANCES.is_cuda and m.NEIGHBOURS.is_cuda
