"""k-means|| seeding (ops.kmeans.min_dist / sample / recluster) on CPU tensors,
the executable specification, against plain float64 numpy, its argument checks,
and examples/KMeans with init_method="kmeans||" through the SPMD engine at W = 1.

Bounds (ops/kmeans.py; u = 2^-24, E_i as in test_kmeans.py with max_j over the
candidates):  B_i = E_i + gamma_{d+2} |x_i|^2 + 2 u (D_i + E_i).  After one call
|mind_i - D_i| <= B_i; over several calls D64[i, near_i] is within 2 B_i of the
float64 minimum and near_i is the float64 argmin wherever the margin exceeds
2 B_i (at most 1 % of the points have a smaller one: asserted on the reference
alone); phi is the float64 sum of mind to within gamma'_n sum mind, u' = 2^-53.
"""
import numpy as np
import pytest
import torch

from test_kmeans import U, blobs, gamma, run_job

SPEC_SHAPES = [(17, 5, 17), (65, 64, 33), (1000, 130, 15)]
JOB_SEED = 7  # naive's smallest selection margin at this seed is 2.5e-3 (3000 points, dim 6, k 5)


def seed_reference(X, C):
    """float64 distances of float32 (or widened bf16) points, and the bounds above."""
    X64, C64 = X.astype(np.float64), C.astype(np.float64)
    d = X.shape[1]
    D = np.concatenate([((X64[i:i + 256, None, :] - C64[None]) ** 2).sum(-1) for i in range(0, len(X), 256)])
    nx = np.linalg.norm(X64, axis=1)
    E = 2 * gamma(d + 2) * (nx + np.linalg.norm(C64, axis=1).max()) ** 2
    B = E + gamma(d + 2) * nx ** 2 + 2 * U * (D.min(1) + E)
    two = np.partition(D, 1, axis=1)[:, :2] if len(C) > 1 else np.stack([D[:, 0], np.full(len(X), np.inf)], 1)
    clear = two[:, 1] - two[:, 0] > 2 * B
    assert (~clear).mean() <= 0.01, "inputs: too many near-ties for the label rule"
    return dict(D=D, B=B, clear=clear)


def check_min_dist(ref, mind, near, phi, fresh):
    D, B = ref["D"], ref["B"]
    n = len(D)
    mind, near = mind.cpu().numpy().astype(np.float64), near.cpu().numpy().astype(np.int64)
    assert near.min() >= 0 and near.max() < D.shape[1]
    err = np.abs(mind - D.min(1))
    print("mind: worst error / bound", (err / B).max() if n else 0.0)
    assert (err <= (B if fresh else 2 * B)).all()
    assert (D[np.arange(n), near] <= D.min(1) + 2 * B).all()
    assert (near[ref["clear"]] == D.argmin(1)[ref["clear"]]).all()
    total = mind.sum()
    assert abs(float(phi.cpu()[0]) - total) <= n * 2.0 ** -53 / (1 - n * 2.0 ** -53) * total


def run_min_dist(dev, X, C, ref):
    """One call from fresh state, then two calls over the halves of C with base."""
    from lua_mapreduce_1_amd.ops import kmeans as K
    x, c = X.to(dev), torch.from_numpy(C).to(dev)
    mind, near, phi = K.min_dist(x, c)
    assert mind.dtype == torch.float32 and near.dtype == torch.int32 and phi.dtype == torch.float64
    check_min_dist(ref, mind, near, phi, fresh=True)
    h = (len(C) + 1) // 2
    m2, n2, p2 = K.min_dist(x, c[:h].contiguous())
    if h < len(C):
        m3, n3, p2 = K.min_dist(x, c[h:].contiguous(), m2, n2, base=h)
        assert m3 is m2 and n3 is n2
    check_min_dist(ref, m2, n2, p2, fresh=False)
    return phi


@pytest.mark.parametrize("n,d,m", SPEC_SHAPES)
def test_min_dist_specification(n, d, m):
    X, C = blobs(n, d, m)
    run_min_dist(torch.device("cpu"), torch.from_numpy(X), C, seed_reference(X, C))


def test_hash_is_uniform_enough():
    from lua_mapreduce_1_amd.ops import kmeans as K
    n = 1 << 16
    idx, rows = K.sample(torch.zeros(n, 1), torch.ones(n), float(n), 1024, 0, 0)
    assert abs(len(idx) - 1024) <= 192  # 6 sigma of Binomial(2^16, 2^-6)
    assert (idx[1:] > idx[:-1]).all() and rows.shape == (len(idx), 1)


def seed_job_checks(device, n, dim, k, seed):
    """The k-means|| job against naive: shared with the GPU test."""
    from lua_mapreduce_1_amd.examples import KMeans as ex
    want = ex.naive(ex.make_points(seed, n, dim, k, 4), k, dim, seed=seed, init_method="kmeans||")
    assert want["seed_margin"].min() > 1e-4, "inputs: a selection within rounding of its threshold"
    runs = {}
    for nsplits in (4, 1):
        args = {"files": "synthetic", "n": n, "nsplits": nsplits, "dim": dim, "k": k, "seed": seed,
                "init_method": "kmeans||"}
        m, _res = run_job(device, args)
        runs[nsplits] = [i.copy() for i in m.SEED_INFO["indices"]]
    assert len(runs[4]) == len(want["seed_indices"]) == len(runs[1])
    for got, one, ref in zip(runs[4], runs[1], want["seed_indices"]):
        assert np.array_equal(got, ref) and np.array_equal(one, ref)
    info = m.SEED_INFO
    assert int(info["weights"].sum()) == n and len(m.SEED_HISTORY) == 6 and 1 <= len(m.HISTORY) <= 20
    assert [h["candidates"] for h in m.SEED_HISTORY][-1] == len(info["candidates"]) == len(info["weights"])
    return m, want


def test_job_cpu_w1_against_naive():
    from lua_mapreduce_1_amd.ops import kmeans as K
    m, want = seed_job_checks(torch.device("cpu"), 3000, 6, 5, JOB_SEED)
    info = m.SEED_INFO
    assert np.array_equal(info["seeds"], K.recluster(info["candidates"], info["weights"], 5, JOB_SEED).numpy())
    assert np.array_equal(info["weights"], want["seed_weights"]) and len(m.HISTORY) == len(want["history"])
    got = m.CENTROIDS.numpy()
    assert (np.linalg.norm(got - want["centroids"], axis=1) <= 1e-4 * np.linalg.norm(want["centroids"], axis=1)).all()


def test_default_init_is_unchanged():
    from lua_mapreduce_1_amd.examples import KMeans as ex
    splits = ex.make_points(3, 3000, 6, 5, 3)
    m, res = run_job(torch.device("cpu"), {"files": "synthetic", "n": 3000, "nsplits": 3, "k": 5, "dim": 6, "seed": 3})
    want = ex.naive(splits, 5, 6, seed=3)
    assert len(m.HISTORY) == len(want["history"]) and 1 < len(m.HISTORY) <= 20 and m.SEED_HISTORY == []
    got = m.CENTROIDS.numpy()
    assert (np.linalg.norm(got - want["centroids"], axis=1) <= 1e-4 * np.linalg.norm(want["centroids"], axis=1)).all()
    assert int(m.rejoin_counts(res.tensors["COUNTS"]).sum()) == 3000


def _bad_calls():
    from lua_mapreduce_1_amd.ops import kmeans as K
    X, one = torch.zeros(4, 8), torch.ones(4)
    return {
        "m16385": (lambda: K.min_dist(X, torch.zeros(16385, 8)), ValueError),
        "fp64-C": (lambda: K.min_dist(X, torch.zeros(2, 8, dtype=torch.float64)), TypeError),
        "mind-shape": (lambda: K.min_dist(X, torch.zeros(2, 8), mind=torch.ones(5)), ValueError),
        "near-dtype": (lambda: K.min_dist(X, torch.zeros(2, 8), near=torch.zeros(4, dtype=torch.int64)), ValueError),
        "sample-mind-fp64": (lambda: K.sample(X, one.double(), 1.0, 2, 0, 0), TypeError),
        "sample-mind-shape": (lambda: K.sample(X, torch.ones(3), 1.0, 2, 0, 0), ValueError),
        "recluster-k": (lambda: K.recluster(torch.zeros(3, 2), [1, 0, 2], 3, 0), ValueError),
    }


@pytest.mark.parametrize("case", ["m16385", "fp64-C", "mind-shape", "near-dtype", "sample-mind-fp64",
                                  "sample-mind-shape", "recluster-k"])
def test_argument_checks(case):
    call, exc = _bad_calls()[case]
    with pytest.raises(exc):
        call()
