"""ops.kmeans on CPU tensors (the executable specification), its argument
checks, and examples/KMeans through the SPMD engine's tensor plane at W = 1.

The reference is plain float64 numpy.  With u = 2^-24 and gamma_m = m u / (1 - m u):

* labels: the path under test minimises an fp32 score |c|^2 - 2 x.c — two
  length-d fma chains and a subtract, each score off by at most
  gamma_{d+2} (|x| + |c|)^2 — so D64[i, label_i] <= min_j D64[i, j] + E_i with
  E_i = 2 gamma_{d+2} (|x_i| + max_j |c_j|)^2, and the label EQUALS the float64
  argmin wherever the float64 margin (second best - best) exceeds E_i.  The
  inputs are such that at most 1 % of the points have a smaller margin
  (asserted on the reference alone, before any result is looked at).
* counts: exact.  sums (over the labels the path returned): n_j additions in
  any order, |sums - ref| <= 2 gamma_{n_j} sum_members |x|.
* cost: per point max(0, fl(|x|^2) + score): the score is within E_i of the
  true minimum, fl(|x|^2) within gamma_{d+2} |x|^2, the final add and the sum
  within gamma_n of the total: sum_i (E_i + gamma_{d+2} |x_i|^2) + gamma_n cost_ref.
"""
import numpy as np
import pytest
import torch

U = 2.0 ** -24
KM = "lua_mapreduce_1_amd.examples.KMeans"


def gamma(m):
    return m * U / (1 - m * U)


def blobs(n, d, k, seed=0):
    rng = np.random.default_rng(seed)
    C = rng.normal(0, 10, (k, d)).astype(np.float32)
    X = (C[rng.integers(0, k, n)] + rng.normal(0, 1, (n, d))).astype(np.float32)
    return X, C


def reference(X, C):
    X64, C64 = X.astype(np.float64), C.astype(np.float64)
    d = X.shape[1]
    D = np.concatenate([((X64[i:i + 256, None, :] - C64[None]) ** 2).sum(-1) for i in range(0, len(X), 256)])
    nx = np.linalg.norm(X64, axis=1)
    E = 2 * gamma(d + 2) * (nx + np.linalg.norm(C64, axis=1).max()) ** 2
    two = np.partition(D, 1, axis=1)[:, :2] if len(C) > 1 else np.stack([D[:, 0], np.full(len(X), np.inf)], 1)
    clear = two[:, 1] - two[:, 0] > E
    assert (~clear).mean() <= 0.01, "inputs: too many near-ties for the label rule"
    return dict(X=X64, D=D, E=E, clear=clear, nx=nx, k=len(C))


def check(ref, sums, counts, cost, labels):
    X, D, E, k = ref["X"], ref["D"], ref["E"], ref["k"]
    n, d = X.shape
    lab = labels.cpu().numpy().astype(np.int64)
    assert lab.min() >= 0 and lab.max() < k
    assert (D[np.arange(n), lab] <= D.min(1) + E).all()
    assert (lab[ref["clear"]] == D.argmin(1)[ref["clear"]]).all()
    cnt = np.bincount(lab, minlength=k)
    assert (counts.cpu().numpy() == cnt).all()
    want, mass = np.zeros((k, d)), np.zeros((k, d))
    np.add.at(want, lab, X)
    np.add.at(mass, lab, np.abs(X))
    err = np.abs(sums.cpu().numpy() - want)
    print("sums: worst error / bound", (err / np.maximum(2 * gamma(cnt)[:, None] * mass, 1e-300)).max())
    assert (err <= 2 * gamma(cnt)[:, None] * mass).all()
    cost_ref = D.min(1).sum()
    bound = (E + gamma(d + 2) * ref["nx"] ** 2).sum() + gamma(n) * cost_ref
    print("cost: error", abs(float(cost.cpu()[0]) - cost_ref), "bound", bound)
    assert abs(float(cost.cpu()[0]) - cost_ref) <= bound


@pytest.mark.parametrize("n,d,k", [(17, 5, 17), (65, 64, 33), (1000, 130, 15)])
def test_cpu_specification(n, d, k):
    from lua_mapreduce_1_amd.ops import kmeans as K
    X, C = blobs(n, d, k)
    ref = reference(X, C)
    sums, counts, cost, lab = K.step(torch.from_numpy(X), torch.from_numpy(C), labels=True)
    check(ref, sums, counts, cost, lab)
    assert lab.dtype == torch.int32 and torch.equal(K.assign(torch.from_numpy(X), torch.from_numpy(C)), lab)


@pytest.mark.parametrize("X,C,exc", [
    (torch.zeros(4, 513), torch.zeros(2, 513), ValueError),
    (torch.zeros(4, 8), torch.zeros(4097, 8), ValueError),
    (torch.zeros(4, 8, dtype=torch.float64), torch.zeros(2, 8), TypeError),
    (torch.zeros(8, 4).t(), torch.zeros(2, 8), ValueError),
], ids=["d513", "k4097", "fp64", "strided"])
def test_argument_checks(X, C, exc):
    from lua_mapreduce_1_amd.ops import kmeans as K
    with pytest.raises(exc):
        K.step(X, C)
    with pytest.raises(exc):
        K.assign(X, C)


def run_job(device, args):
    import importlib
    from lua_mapreduce_1_amd import spmd
    m = importlib.import_module(KM)
    eng = spmd(dict(taskfn=KM, mapfn=KM, partitionfn=KM, reducefn=KM, finalfn=KM, init_args=args), device=device)
    assert eng.plane_kind == "tensor"
    return m, eng.run()


def test_job_cpu_w1_against_naive(tmp_path):
    from lua_mapreduce_1_amd.examples import KMeans as ex
    splits = ex.make_points(3, 3000, 6, 5, 3)
    files = []
    for i, s in enumerate(splits):
        files.append(str(tmp_path / f"points{i}.f32"))
        s.astype("<f4").tofile(files[-1])
    m, res = run_job(torch.device("cpu"), {"files": files, "k": 5, "dim": 6, "seed": 7})
    want = ex.naive(splits, 5, 6, seed=7)
    assert len(m.HISTORY) == len(want["history"]) and 1 < len(m.HISTORY) < 20
    got = m.CENTROIDS.numpy()
    assert (np.linalg.norm(got - want["centroids"], axis=1) <= 1e-4 * np.linalg.norm(want["centroids"], axis=1)).all()
    assert int(m.rejoin_counts(res.tensors["COUNTS"]).sum()) == 3000
    big = torch.tensor([(1 << 24) + 1, 0, (1 << 39) + 12345, (1 << 20) - 1, 1 << 20])
    assert torch.equal(m.rejoin_counts(m.split_counts(big)), big)
    assert torch.equal(m.rejoin_counts(m.split_counts(big + (1 << 43))), big + (1 << 43))
    assert torch.equal(m.rejoin_counts(sum(m.split_counts(big) for _ in range(16))), 16 * big)  # W = 16 sums
