"""The mixture kernels (csrc/hip/gmm.hip) against the float64 numpy reference of
test_gmm.py (every bound is the contract's, derived in ops/gmm.py), at the
smallest shapes at which each part can go wrong, and examples/GaussianMixture
end to end on cuda:0."""
import numpy as np
import pytest
import torch

from test_gmm import RUN, U, UP, check, check_job, gamma, mixture, reference, tens

pytestmark = pytest.mark.gpu

SHAPES = [(1, 1, 1), (15, 3, 2), (17, 5, 17),
          (130, 16, 64),     # exactly one component tile
          (300, 33, 65),     # odd d: a column-tile tail; a second component tile with one live row
          (257, 128, 3),     # d at the limit
          (300, 4, 4096),    # k at the limit
          (100_000, 8, 5),   # hundreds of slabs, five contended components
          (300_000, 2, 3)]   # past 4 workgroups per CU: several super-tiles per slab, accumulators carried across


def run(gpu, X, w, M, V, **acc):
    """estep(labels=True) on the device and the reference against the A, b that device returned."""
    from lua_mapreduce_1_amd.ops import gmm as G
    t = tens(X, w, M, V, device=gpu)
    Ab = G.prepare(*t[1:])
    A_cpu, b_cpu = G.prepare(*tens(w, M, V))
    assert torch.equal(Ab[0].cpu(), A_cpu)
    assert ((Ab[1].cpu().double() - b_cpu.double()).abs() <= 2 * U * b_cpu.double().abs()).all()  # one fp32 ulp
    return G.estep(*t, labels=True, **acc), Ab, t


@pytest.mark.parametrize("n,d,k", SHAPES)
def test_estep_shapes(gpu, n, d, k):
    from lua_mapreduce_1_amd.ops import gmm as G
    X, w, M, V = mixture(n, d, k)
    out, Ab, t = run(gpu, X, w, M, V)
    ref = reference(X, w, M, V, Ab=Ab)
    check(ref, *out)
    nk, _s1, _s2, ll, logp, lab = out
    assert torch.equal(G.score_samples(*t), logp) and torch.equal(G.predict(*t), lab)
    assert abs(float(nk.sum()) - n) <= ref["rho"].sum() + gamma(RUN) * n
    lp = logp.double().cpu().numpy()
    assert abs(float(ll) - lp.sum()) <= gamma(n, UP) * np.abs(lp).sum()


def test_extremes_stay_finite(gpu):
    X, w, M, V = mixture(500, 6, 4, seed=1)
    sd = np.sqrt(V)
    M[3] = M[3] + 1e3 * sd[3]                       # a component no point is near
    X[:20] = M[:3].mean(0) + 50 * sd.max(0) * np.where(np.arange(6) % 2, 1, -1)  # outliers, >= 50 sd from every mean
    out, Ab, _t = run(gpu, X, w, M, V)
    ref = reference(X, w, M, V, Ab=Ab, label_rule=False)  # the far component's |b| makes every e_i large
    assert all(torch.isfinite(o).all() for o in out[:5])
    check(ref, *out[:5])  # covers the far component's row of s1 and the outliers' logp, bound by bound
    assert np.abs(out[1][3].cpu().numpy()).max() <= 1e-30 and ref["logp"][:20].max() < -1000


def test_ties_share_and_go_to_the_lowest_index(gpu):
    X, w, M, V = mixture(500, 20, 9, seed=2)
    for hi, lo in ((7, 3), (1, 0)):
        M[hi], V[hi], w[hi] = M[lo], V[lo], w[lo]
    (nk, _s1, _s2, _ll, _logp, lab), Ab, _t = run(gpu, X, w / w.sum(), M, V)
    ref = reference(X, w / w.sum(), M, V, Ab=Ab, label_rule=False)  # the twins tie exactly: margin 0 by design
    lab = lab.cpu().numpy()
    assert not np.isin(lab, (7, 1)).any() and np.isin(lab, (3, 0)).any()
    nk = nk.cpu().numpy()
    for hi, lo in ((7, 3), (1, 0)):
        assert abs(nk[hi] - nk[lo]) <= 2 * (ref["rho"] * ref["R"][:, lo]).sum() + 2 * gamma(RUN) * ref["nk"][lo]


def test_accumulates_into(gpu):
    X, w, M, V = mixture(3000, 24, 11, seed=3)
    (nk, s1, s2, ll, lp1, l1), Ab, _t = run(gpu, X[:1700], w, M, V)
    out2, _Ab, _t = run(gpu, X[1700:], w, M, V, nk=nk, s1=s1, s2=s2, ll=ll)
    assert all(a is b for a, b in zip(out2[:4], (nk, s1, s2, ll)))
    check(reference(X, w, M, V, Ab=Ab), nk, s1, s2, ll, torch.cat([lp1, out2[4]]), torch.cat([l1, out2[5]]))


def test_job_gpu_against_naive(gpu):
    from lua_mapreduce_1_amd.examples import KMeans as km
    args = {"files": "synthetic", "n": 20_000, "nsplits": 4, "dim": 16, "k": 8, "seed": 5}
    m, res = check_job(gpu, km.make_points(5, 20_000, 16, 8, 4), args)
    assert res.tensors["S1"].is_cuda and m.MEANS.is_cuda and m.WEIGHTS.is_cuda and m.VARIANCES.is_cuda
