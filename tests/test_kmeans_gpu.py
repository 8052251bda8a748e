"""The fused k-means kernel (csrc/hip/kmeans.hip) against the float64 numpy
reference of test_kmeans.py (bounds derived there), at the smallest shapes at
which each part of it can go wrong, and examples/KMeans end to end on cuda:0."""
import numpy as np
import pytest
import torch

from test_kmeans import blobs, check, reference, run_job

pytestmark = pytest.mark.gpu

SHAPES = [(1, 1, 1), (15, 3, 2), (17, 5, 17), (64, 4, 16), (65, 64, 33),  # tails everywhere, one and two MFMA tiles
          (1000, 130, 15),   # d no multiple of 4, two d-chunks
          (257, 512, 3),     # d at the limit
          (300, 4, 4096),    # k at the limit, most clusters empty
          (100_000, 8, 5)]   # several super-tiles per workgroup, five contended clusters


def run_step(gpu, X, C, **acc):
    from lua_mapreduce_1_amd.ops import kmeans as K
    return K.step(torch.from_numpy(X).to(gpu), torch.from_numpy(C).to(gpu), labels=True, **acc)


@pytest.mark.parametrize("n,d,k", SHAPES)
def test_step_shapes(gpu, n, d, k):
    from lua_mapreduce_1_amd.ops import kmeans as K
    X, C = blobs(n, d, k)
    ref = reference(X, C)
    sums, counts, cost, lab = run_step(gpu, X, C)
    check(ref, sums, counts, cost, lab)
    assert (sums[counts == 0] == 0).all()
    assert torch.equal(K.assign(torch.from_numpy(X).to(gpu), torch.from_numpy(C).to(gpu)), lab)


@pytest.mark.parametrize("d", [128, 512])
@pytest.mark.parametrize("over", [0, 1], ids=["lds", "direct"])
def test_both_sides_of_the_lds_limit(gpu, d, over):
    from lua_mapreduce_1_amd.ops import kmeans as K
    k = K.lds_limit(d) + over
    assert 1 <= k <= 4096
    X, C = blobs(2000, d, k)
    ref = reference(X, C)
    check(ref, *run_step(gpu, X, C))


def test_ties_go_to_the_lowest_index(gpu):
    X, C = blobs(500, 20, 9, seed=1)
    C[7], C[1] = C[3], C[0]
    lab = run_step(gpu, X, C)[3].cpu().numpy()
    assert not np.isin(lab, (7, 1)).any() and np.isin(lab, (3, 0)).any()


def test_accumulates_into(gpu):
    X, C = blobs(3000, 24, 11, seed=2)
    ref = reference(X, C)
    s, c, q, l1 = run_step(gpu, X[:1700], C)
    s2, c2, q2, l2 = run_step(gpu, X[1700:], C, sums=s, counts=c, cost=q)
    assert s2 is s and c2 is c and q2 is q
    check(ref, s, c, q, torch.cat([l1, l2]))


def test_job_gpu_against_naive(gpu):
    from lua_mapreduce_1_amd.examples import KMeans as ex
    args = {"files": "synthetic", "n": 20_000, "nsplits": 4, "dim": 16, "k": 8, "seed": 5}
    m, res = run_job(gpu, args)
    splits = ex.make_points(5, 20_000, 16, 8, 4)
    want = ex.naive(splits, 8, 16, seed=5)
    assert res.tensors["SUMS"].is_cuda and m.CENTROIDS.is_cuda
    assert len(m.HISTORY) == len(want["history"])
    got = m.CENTROIDS.cpu().numpy()
    assert (np.linalg.norm(got - want["centroids"], axis=1) <= 1e-4 * np.linalg.norm(want["centroids"], axis=1)).all()
    X = np.concatenate(splits)
    ref = reference(X, m.CENTROIDS.cpu().numpy())
    lab = m.predict(X).cpu().numpy().astype(np.int64)
    assert (ref["D"][np.arange(len(X)), lab] <= ref["D"].min(1) + ref["E"]).all()
    assert (lab[ref["clear"]] == ref["D"].argmin(1)[ref["clear"]]).all()
