"""ops.gmm on CPU tensors (the executable specification), its argument checks,
and examples/GaussianMixture through the tensor plane at W = 1.

The reference is plain float64 numpy evaluated with the fp32 A, b that
``prepare`` returned, and ``check`` asserts every bound of the contract in
ops/gmm.py's docstring (u = 2^-24) over every point and every entry; only the
label rule is restricted, to the points whose float64 margin exceeds 2 e_i.
"""
import numpy as np
import pytest
import torch

U, UP = 2.0 ** -24, 2.0 ** -53
GM = "lua_mapreduce_1_amd.examples.GaussianMixture"
RUN = 4096


def gamma(m, u=U):
    return m * u / (1 - m * u)


def mixture(n, d, k, seed=0):
    rng = np.random.default_rng(seed)
    M = rng.normal(0, 2, (k, d))
    sd = rng.uniform(0.5, 1.5, (k, d))
    w = rng.uniform(0.5, 1.5, k)
    w /= w.sum()
    z = rng.choice(k, n, p=w)
    X = M[z] + sd[z] * rng.normal(0, 1, (n, d))
    return tuple(np.ascontiguousarray(a, dtype=np.float32) for a in (X, w, M, sd * sd))


def tens(*arrays, device="cpu"):
    return tuple(torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).to(device) for a in arrays)


def reference(X, w, M, V, Ab=None, label_rule=True):
    from lua_mapreduce_1_amd.ops import gmm as G
    assert G.RUN == RUN
    A, b = (t.cpu().numpy().astype(np.float64) for t in (Ab or G.prepare(*tens(w, M, V))))
    n, d = X.shape
    k = len(b)
    x, x2 = X.astype(np.float64), (X * X).astype(np.float64)
    Z = np.concatenate([x, x2], 1)
    S = Z @ A.T + b
    top = S.max(1)
    logp = top + np.log(np.exp(S - top[:, None]).sum(1))
    e = gamma(2 * d + 2) * (np.abs(b) + np.abs(Z) @ np.abs(A).T).max(1)
    B = 2 * e + (k + 8) * U + 4 * U * np.abs(logp)
    two = np.sort(S, 1)[:, -2:] if k > 1 else np.stack([np.full(n, -np.inf), S[:, 0]], 1)
    clear = two[:, 1] - two[:, 0] > 2 * e
    assert not label_rule or clear.mean() >= 0.95, "inputs: too many near-ties for the label rule"
    R = np.exp(S - logp[:, None])
    with np.errstate(over="ignore"):  # a collapsed component: rho = inf, the bound says nothing there
        rho = np.expm1(2 * B) + 4 * U
    return dict(X=x, X2=x2, S=S, logp=logp, R=R, e=e, B=B, rho=rho, clear=clear, k=k,
                nk=R.sum(0), s1=R.T @ x, s2=R.T @ x2)


def stat_bounds(ref):
    """The contract's bounds on (nk, s1, s2)."""
    n = len(ref["X"])
    wR = (ref["rho"] + gamma(RUN) + gamma(n, UP))[:, None] * ref["R"]
    floor = n * 2.0 ** -126
    ax = np.abs(ref["X"])
    return wR.sum(0) + floor, wR.T @ ax + floor * ax.max(initial=0), wR.T @ ref["X2"] + floor * ref["X2"].max(initial=0)


def check(ref, nk, s1, s2, ll, logp, labels=None):
    got = logp.cpu().numpy().astype(np.float64)
    err = np.abs(got - ref["logp"])
    print("logp: worst error / bound", (err / ref["B"]).max(initial=0))
    assert (err <= ref["B"]).all()
    if labels is not None:
        lab = labels.cpu().numpy().astype(np.int64)
        assert lab.min(initial=0) >= 0 and lab.max(initial=0) < ref["k"]
        assert (lab[ref["clear"]] == ref["S"].argmax(1)[ref["clear"]]).all()
    for name, t, bound in zip(("nk", "s1", "s2"), (nk, s1, s2), stat_bounds(ref)):
        err = np.abs(t.cpu().numpy() - ref[name])
        print(name, ": worst error / bound", (err / np.maximum(bound, 1e-300)).max(initial=0))
        assert np.isfinite(t.cpu().numpy()).all() and (err <= bound).all(), name
    n = len(got)
    ll_bound = ref["B"].sum() + gamma(n, UP) * np.abs(ref["logp"]).sum()
    print("ll: error", abs(float(ll.cpu()[0]) - ref["logp"].sum()), "bound", ll_bound)
    assert abs(float(ll.cpu()[0]) - ref["logp"].sum()) <= ll_bound


@pytest.mark.parametrize("n,d,k", [(17, 5, 17), (300, 33, 65), (257, 128, 3)])
def test_cpu_specification(n, d, k):
    from lua_mapreduce_1_amd.ops import gmm as G
    X, w, M, V = mixture(n, d, k)
    A, b = G.prepare(*tens(w, M, V))
    M64, V64 = M.astype(np.float64), V.astype(np.float64)
    assert np.array_equal(A.numpy(), np.concatenate([M64 / V64, -0.5 / V64], 1).astype(np.float32))
    b64 = np.log(w.astype(np.float64)) - 0.5 * (np.log(2 * np.pi * V64) + M64 * M64 / V64).sum(1)
    assert (np.abs(b.numpy() - b64) <= U * np.abs(b64)).all()
    ref = reference(X, w, M, V)
    out = G.estep(*tens(X, w, M, V), labels=True)
    check(ref, *out)
    assert out[5].dtype == torch.int32 and torch.equal(G.predict(*tens(X, w, M, V)), out[5])
    assert torch.equal(G.score_samples(*tens(X, w, M, V)), out[4])


def _params(d=8, k=2):
    return torch.zeros(4, d), torch.full((k,), 1.0 / k), torch.zeros(k, d), torch.ones(k, d)


@pytest.mark.parametrize("edit,exc", [
    (lambda p: (p[0].double(),) + p[1:], TypeError),
    (lambda p: (p[0][0],) + p[1:], ValueError),
    (lambda p: (torch.zeros(8, 4).t(),) + p[1:], ValueError),
    (lambda p: _params(d=129), ValueError),
    (lambda p: _params(k=4097), ValueError),
    (lambda p: p[:3] + (p[3].clone().index_fill_(0, torch.tensor([1]), 0.0),), ValueError),
    (lambda p: (p[0], torch.tensor([1.0, 0.0])) + p[2:], ValueError),
], ids=["fp64", "rank", "strided", "d129", "k4097", "zero-variance", "zero-weight"])
def test_argument_checks(edit, exc):
    from lua_mapreduce_1_amd.ops import gmm as G
    for fn in (G.estep, G.score_samples, G.predict):
        with pytest.raises(exc):
            fn(*edit(_params()))


def run_job(device, args):
    import importlib
    from lua_mapreduce_1_amd import spmd
    m = importlib.import_module(GM)
    eng = spmd(dict(taskfn=GM, mapfn=GM, partitionfn=GM, reducefn=GM, finalfn=GM, init_args=args), device=device)
    assert eng.plane_kind == "tensor"
    return m, eng.run()


def check_job(device, splits, args):
    """The three assertions on the job: one M-step against ``naive``, EM's
    monotone log-likelihood, and the last ll against the reference at the final
    parameters.  ``naive`` uses the plain formula, the contract the fp32 A, b:
    rounding them moves a score by at most e_i / (2d + 2), which the 2 e_i the
    bounds allow beside the chain's own e_i covers."""
    from lua_mapreduce_1_amd.examples import GaussianMixture as ex
    k, dim, J = args["k"], args["dim"], len(splits)
    X = np.concatenate(splits)
    plane = gamma(J + 1)  # every job's float64 result rounded to fp32, then J fp32 adds
    m, _res = run_job(device, {**args, "max_iters": 2})
    want = ex.naive(splits, k, dim, max_iters=2, seed=args["seed"])
    ref = reference(X, *ex.initial_parameters(splits, k, dim, args["seed"], 1e-6), label_rule=False)
    dnk, ds1, ds2 = (bnd + plane * mass for bnd, mass in
                     zip(stat_bounds(ref), (ref["nk"], ref["R"].T @ np.abs(ref["X"]), ref["s2"])))
    nk = (ref["nk"] - dnk)[:, None]
    assert (nk > 0).all()
    mu, ex2 = ref["s1"] / ref["nk"][:, None], ref["s2"] / ref["nk"][:, None]
    dmu = (ds1 + np.abs(mu) * dnk[:, None]) / nk
    dvar = (ds2 + ex2 * dnk[:, None]) / nk + 2 * np.abs(mu) * dmu + dmu ** 2
    dw = (dnk + ref["nk"] / len(X) * dnk.sum()) / (len(X) - dnk.sum())
    for got, exp, bound in ((m.WEIGHTS, want["weights"], dw), (m.MEANS, want["means"], dmu),
                            (m.VARIANCES, want["variances"], dvar)):
        assert (np.abs(got.cpu().numpy() - exp) <= bound + U * np.abs(exp)).all()

    m, res = run_job(device, args)
    final = reference(X, *(p.cpu().numpy() for p in (m.WEIGHTS, m.MEANS, m.VARIANCES)),
                      Ab=m.G.prepare(m.WEIGHTS, m.MEANS, m.VARIANCES), label_rule=False)
    lls = np.array([h["ll"] for h in m.HISTORY])
    assert 2 < len(lls) <= 50
    slack = 2 * max(ref["B"].sum(), final["B"].sum()) + plane * np.abs(lls).max()
    assert (np.diff(lls) >= -slack).all()
    assert abs(lls[-1] - final["logp"].sum()) <= final["B"].sum() + plane * abs(final["logp"]).sum()
    return m, res


def test_job_cpu_w1_against_naive(tmp_path):
    from lua_mapreduce_1_amd.examples import KMeans as km
    splits = km.make_points(3, 3000, 6, 5, 3)
    files = []
    for i, s in enumerate(splits):
        files.append(str(tmp_path / f"points{i}.f32"))
        s.astype("<f4").tofile(files[-1])
    m, _res = check_job(torch.device("cpu"), splits, {"files": files, "k": 5, "dim": 6, "seed": 7})
    X = np.concatenate(splits)
    assert m.predict(X).shape == (3000,) and m.score_samples(X).dtype == torch.float32
