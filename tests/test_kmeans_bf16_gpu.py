"""The bf16 k-means kernels (csrc/hip/kmeans_bf16.hip) against the float64 numpy
reference of test_kmeans_bf16.py (bounds derived there), at the smallest shapes
at which each part can go wrong, and examples/KMeans on bf16 points on cuda:0."""
import numpy as np
import pytest
import torch

from test_kmeans import blobs, check, run_job
from test_kmeans_bf16 import case, mixed, reference

pytestmark = pytest.mark.gpu

SHAPES = [(1, 1, 1), (17, 5, 17), (65, 64, 33),
          (300, 40, 70),     # d no multiple of 8, two centroid tiles with a tail
          (257, 512, 3),     # d at the limit
          (300, 4, 4096),    # k at the limit, most clusters empty
          (100_000, 8, 5),   # several super-tiles per workgroup, five contended clusters
          (70, 32, 9), (70, 33, 9), (300, 65, 9), (140, 128, 40), (140, 129, 40),  # both sides of every
          (140, 256, 9), (140, 257, 9)]                                            # d boundary ((65, 64, 33) above)
CASES = [s + (3,) for s in SHAPES] + [s + (T,) for T in (1, 2) for s in ((17, 5, 17), (300, 40, 70), (1000, 130, 15))]


def run_step(gpu, X, C, T, **acc):
    from lua_mapreduce_1_amd.ops import kmeans as K
    return K.step(X.to(gpu), C.to(gpu), labels=True, terms=T, **acc)


@pytest.mark.parametrize("n,d,k,T", CASES)
def test_step_shapes(gpu, n, d, k, T):
    from lua_mapreduce_1_amd.ops import kmeans as K
    X, C, ref = case(n, d, k, T)
    sums, counts, cost, lab = run_step(gpu, X, C, T)
    check(ref, sums, counts, cost, lab)
    assert (sums[counts == 0] == 0).all()
    assert torch.equal(K.assign(X.to(gpu), C.to(gpu), terms=T), lab)


@pytest.mark.parametrize("d", [128, 512])
@pytest.mark.parametrize("over", [0, 1], ids=["lds", "direct"])
def test_both_sides_of_the_lds_limit(gpu, d, over):
    from lua_mapreduce_1_amd.ops import kmeans as K
    k = K.lds_limit(d, torch.bfloat16) + over
    assert 1 <= k <= 4096
    X, C, ref = case(2000, d, k, 3)
    check(ref, *run_step(gpu, X, C, 3))


@pytest.mark.parametrize("T", [1, 2, 3])
def test_split_is_the_specification(gpu, T):
    from lua_mapreduce_1_amd.ops import kmeans as K
    C = mixed()
    P, cn = K.split_centroids(C.to(gpu), T)
    P0, cn0 = K.split_centroids(C, T)
    assert torch.equal(P.cpu().view(torch.int16), P0.view(torch.int16))
    assert torch.equal(cn.cpu().view(torch.int32), cn0.view(torch.int32))
    assert T < 3 or torch.equal(P.cpu().double().sum(0), C.double())


def test_terms_choose_the_centroids(gpu):
    """Points that are clear under both C_1 and C_3 and have different argmins
    follow C_1 at terms=1 and C_3 at terms=3.  One set of (20 000, 4, 64) blobs
    holds 0 to 4 such points (counted on the reference alone, seeds 0..15), so
    the 20 the check wants are gathered over 16 seeds of that shape."""
    found = 0
    for seed in range(16):
        X, C, r1 = case(20_000, 4, 64, 1, seed)
        r3 = case(20_000, 4, 64, 3, seed)[2]
        a1, a3 = r1["D"].argmin(1), r3["D"].argmin(1)
        pick = r1["clear"] & r3["clear"] & (a1 != a3)
        found += int(pick.sum())
        if pick.any():
            assert (run_step(gpu, X, C, 1)[3].cpu().numpy()[pick] == a1[pick]).all()
            assert (run_step(gpu, X, C, 3)[3].cpu().numpy()[pick] == a3[pick]).all()
    assert found >= 20


@pytest.mark.parametrize("d", [1, 4])
def test_the_third_piece_is_used(gpu, d):
    from lua_mapreduce_1_amd.ops import kmeans as K
    C = torch.tensor([1 + 2.0 ** -9 + 2.0 ** -17, 1 + 2.0 ** -9], dtype=torch.float32)[:, None].repeat(1, d).contiguous()
    X = torch.full((64, d), -1.0, dtype=torch.bfloat16)
    P = K.split_centroids(C, 3)[0].float()
    assert torch.equal(P[:2, 0], P[:2, 1]) and (P[2, 0] == 2.0 ** -17).all() and (P[2, 1] == 0).all()
    ref = reference(X.float().numpy(), P.sum(0).numpy(), 3)
    assert ref["clear"].all() and (ref["D"].argmin(1) == 1).all()
    assert (run_step(gpu, X, C, 3)[3] == 1).all()
    assert (run_step(gpu, X, C, 2)[3] == 0).all()  # a tie under C_2: the lowest index


def test_ties_go_to_the_lowest_index(gpu):
    X, C = blobs(500, 20, 9, seed=1)
    C[7], C[1] = C[3], C[0]
    lab = run_step(gpu, torch.from_numpy(X).to(torch.bfloat16), torch.from_numpy(C), 3)[3].cpu().numpy()
    assert not np.isin(lab, (7, 1)).any() and np.isin(lab, (3, 0)).any()


def test_accumulates_into(gpu):
    X, C, ref = case(3000, 24, 11, 3, seed=2)
    s, c, q, l1 = run_step(gpu, X[:1700], C, 3)
    s2, c2, q2, l2 = run_step(gpu, X[1700:], C, 3, sums=s, counts=c, cost=q)
    assert s2 is s and c2 is c and q2 is q
    check(ref, s, c, q, torch.cat([l1, l2]))


def test_job_gpu_against_naive(gpu):
    from lua_mapreduce_1_amd.examples import KMeans as ex
    from lua_mapreduce_1_amd.ops import kmeans as K
    args = {"files": "synthetic", "n": 20_000, "nsplits": 4, "dim": 16, "k": 8, "seed": 5, "point_dtype": "bf16"}
    m, res = run_job(gpu, args)
    splits = [ex.to_bf16(s) for s in ex.make_points(5, 20_000, 16, 8, 4)]
    want = ex.naive(splits, 8, 16, seed=5)
    assert res.tensors["SUMS"].is_cuda and m.CENTROIDS.is_cuda
    assert len(m.HISTORY) == len(want["history"])
    got = m.CENTROIDS.cpu().numpy()
    assert (np.linalg.norm(got - want["centroids"], axis=1) <= 1e-4 * np.linalg.norm(want["centroids"], axis=1)).all()
    X = np.concatenate(splits)
    ref = reference(ex.widen(X), K.split_centroids(m.CENTROIDS.cpu(), 3)[0].float().sum(0).numpy(), 3)
    lab = m.predict(X).cpu().numpy().astype(np.int64)
    assert (ref["D"][np.arange(len(X)), lab] <= ref["D"].min(1) + ref["E"]).all()
    assert (lab[ref["clear"]] == ref["D"].argmin(1)[ref["clear"]]).all()
