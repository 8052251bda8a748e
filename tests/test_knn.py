"""ops.knn on CPU tensors (the executable specification), merge, classify, the
argument checks, and examples/KNN through the tensor plane at W = 1.

``reference`` is plain float64 numpy sorted by (distance, index); given a
result it asserts every rule of the contract in ops/knn.py's docstring
(u = 2^-24) for every query.  Accuracy uses ``B_i`` at the pair's own float64
distance; separation and set equality use ``B_i`` at the query's largest
float64 distance, which bounds every distance they involve.
"""
import numpy as np
import pytest
import torch

U = 2.0 ** -24
KN = "lua_mapreduce_1_amd.examples.KNN"


def reference(Q, X, k, got=None, base=0, min_clear=0.0, exact=False):
    Q64, X64 = Q.astype(np.float64), X.astype(np.float64)
    (q, d), n, m = Q.shape, len(X), min(k, len(X))
    D = np.empty((q, n))
    rows = max(1, (1 << 22) // max(1, n * d))
    for i in range(0, q, rows):
        D[i:i + rows] = ((Q64[i:i + rows, None, :] - X64[None]) ** 2).sum(-1)
    order = np.argsort(D, axis=1, kind="stable")  # stable: the lowest index first among equals
    want_d, want_i = np.full((q, k), np.inf), np.full((q, k), -1, dtype=np.int64)
    want_d[:, :m], want_i[:, :m] = np.take_along_axis(D, order[:, :m], 1), order[:, :m] + base
    g = (d + 2) * U / (1 - (d + 2) * U)
    qn2 = (Q64 ** 2).sum(1)
    E = 2 * g * (np.sqrt(qn2) + np.sqrt((X64 ** 2).sum(1)).max(initial=0.0)) ** 2
    B0 = E + g * qn2 + 2 * U * E
    B = B0 + 2 * U * D.max(1, initial=0.0)
    gap = D[np.arange(q), order[:, k]] - want_d[:, k - 1] if n > k else np.full(q, np.inf)
    ref = dict(D=D, dist=want_d, idx=want_i, B=B, clear=gap > 2 * B)
    if got is None:
        return ref
    dist, idx = (t.cpu().numpy() for t in got)
    assert dist.dtype == np.float32 and idx.dtype == np.int64 and dist.shape == idx.shape == (q, k)
    assert (idx[:, m:] == -1).all() and np.isposinf(dist[:, m:]).all()
    loc, dist = idx[:, :m] - base, dist[:, :m].astype(np.float64)
    assert (loc >= 0).all() and (loc < n).all() and (np.diff(np.sort(loc, 1), axis=1) > 0).all()
    assert (np.diff(dist, axis=1) >= 0).all()
    if exact:
        assert np.array_equal(dist, want_d[:, :m]) and np.array_equal(idx, want_i)
    Dg = np.take_along_axis(D, loc, 1)
    share = np.abs(dist - Dg) / (B0[:, None] + 2 * U * Dg)
    print("worst error / B_i", share.max(initial=0.0), "clear", ref["clear"].mean() if q else 1.0)
    assert (share <= 1).all()
    returned = np.zeros(D.shape, dtype=bool)
    np.put_along_axis(returned, loc, True, 1)
    assert (Dg.max(1, initial=0.0) <= np.where(returned, np.inf, D).min(1, initial=np.inf) + 2 * B).all()
    assert q == 0 or ref["clear"].mean() >= min_clear, "inputs: too many near-ties for the set rule"
    assert np.array_equal(np.sort(loc[ref["clear"]], 1), np.sort(order[ref["clear"], :m], 1))
    return ref


def normal(n, d, q):
    rng = np.random.default_rng(0)
    X = rng.standard_normal((n, d)).astype(np.float32)  # X first
    return rng.standard_normal((q, d)).astype(np.float32), X


def small_ints(n, d, q, kind="rand"):
    """Coordinates in [-8, 8]: every fp32 operation is exact and ties are plentiful."""
    rng = np.random.default_rng(n + d)
    X, Q = (rng.integers(-8, 9, (r, d)).astype(np.float32) for r in (n, q))
    if kind == "sorted":  # descending distance to query 0: every tile passes its threshold
        X = X[np.argsort(-((X - Q[0]) ** 2).sum(1), kind="stable")]
    return Q, np.ascontiguousarray(np.tile(X[:1], (n, 1)) if kind == "same" else X)


def tens(*arrays, device="cpu"):
    return tuple(torch.from_numpy(a).to(device) for a in arrays)


@pytest.mark.parametrize("n,d,q,k", [(200, 5, 130, 16), (65, 64, 129, 16), (300, 130, 17, 64), (17, 5, 3, 64),
                                      (0, 4, 9, 3)])
def test_cpu_specification(n, d, q, k):
    from lua_mapreduce_1_amd.ops import knn as N
    Q, X = normal(n, d, q)
    reference(Q, X, k, N.search(*tens(Q, X), k, base=7), base=7)
    Q, X = small_ints(n, d, q)
    reference(Q, X, k, N.search(*tens(Q, X), k), exact=True)


def test_pieces_merge_and_running_state():
    from lua_mapreduce_1_amd.ops import knn as N
    Q, X = small_ints(500, 6, 40)
    tq, tx = tens(Q, X)
    whole = N.search(tq, tx, 33, base=2 ** 33 + 5)
    reference(Q, X, 33, whole, base=2 ** 33 + 5, exact=True)
    dist = idx = None
    for lo, hi in ((0, 17), (17, 300), (300, 500)):
        dist, idx = N.search(tq, tx[lo:hi].contiguous(), 33, dist, idx, base=2 ** 33 + 5 + lo)
    merged = N.merge(*N.search(tq, tx[:300].contiguous(), 33, base=2 ** 33 + 5),
                     *N.search(tq, tx[300:].contiguous(), 33, base=2 ** 33 + 305))
    for got in ((dist, idx), merged):
        assert torch.equal(got[0], whole[0]) and torch.equal(got[1], whole[1])


def test_classify():
    from lua_mapreduce_1_amd.ops import knn as N
    labels = torch.tensor([2, 2, 1, 1, 0, 3])
    idx = torch.tensor([[0, 1, 2], [2, 0, -1], [5, 4, 3], [3, 2, 0], [-1, -1, -1]])
    got = N.classify(idx, labels, 4)  # a majority; a 1-1 tie: the lowest class; a 3-way tie; a majority; no votes
    assert got.dtype == torch.int32 and got.tolist() == [2, 1, 0, 1, 0]
    with pytest.raises(ValueError):
        N.classify(idx, labels, 3)


@pytest.mark.parametrize("edit,exc", [
    (lambda a: dict(a, Q=a["Q"].double()), TypeError),
    (lambda a: dict(a, X=a["X"][0]), ValueError),
    (lambda a: dict(a, X=torch.zeros(8, 9).t()), ValueError),
    (lambda a: dict(a, X=torch.zeros(9, 7)), ValueError),
    (lambda a: dict(a, Q=torch.zeros(4, 513), X=torch.zeros(9, 513)), ValueError),
    (lambda a: dict(a, k=0), ValueError),
    (lambda a: dict(a, k=65), ValueError),
    (lambda a: dict(a, base=-1), ValueError),
    (lambda a: dict(a, base=2 ** 63 - 5), ValueError),
    (lambda a: dict(a, slabs=0), ValueError),
    (lambda a: dict(a, dist=torch.zeros(4, 3)), ValueError),
    (lambda a: dict(a, dist=torch.zeros(4, 2), idx=torch.zeros(4, 2, dtype=torch.int64)), ValueError),
], ids=["fp64", "rank", "strided", "d-mismatch", "d513", "k0", "k65", "base<0", "base-overflow", "slabs0",
        "dist-alone", "state-shape"])
def test_argument_checks(edit, exc):
    from lua_mapreduce_1_amd.ops import knn as N
    with pytest.raises(exc):
        N.search(**edit(dict(Q=torch.zeros(4, 8), X=torch.zeros(9, 8), k=3)))


def run_job(device, splits, args, queries, k):
    """Run examples/KNN and hold its result to ``naive`` under the contract."""
    import importlib
    from lua_mapreduce_1_amd import spmd
    m = importlib.import_module(KN)
    eng = spmd(dict(taskfn=KN, mapfn=KN, partitionfn=KN, reducefn=KN, finalfn=KN,
                    init_args={**args, "queries": queries, "k": k}), device=device)
    assert eng.plane_kind == "tensor"
    res = eng.run()
    X = np.concatenate(splits)
    ref = reference(queries, X, k, (m.DISTANCES, m.NEIGHBOURS), min_clear=0.85)
    want_d, want_i = m.naive(splits, queries, k)
    assert np.array_equal(want_i, ref["idx"]) and np.array_equal(want_d, ref["dist"])
    assert int(m._km.rejoin_counts(res.tensors["ROWS"])[0]) == len(X)
    return m


def test_job_cpu_w1_against_naive(tmp_path):
    from lua_mapreduce_1_amd.examples import KMeans as km
    splits = km.make_points(3, 3000, 6, 5, 3)
    files = []
    for i, s in enumerate(splits):
        files.append(str(tmp_path / f"points{i}.f32"))
        s.astype("<f4").tofile(files[-1])
    queries = np.random.default_rng(1).normal(0, 10, (50, 6)).astype(np.float32)
    m = run_job(torch.device("cpu"), splits, {"files": files, "dim": 6}, queries, 7)
    assert m.NEIGHBOURS.shape == (50, 7)
    with pytest.raises(RuntimeError):
        m.mapfn(None, None, None)
