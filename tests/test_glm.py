"""ops.glm on CPU tensors (the executable specification), its float64 helpers, the
argument checks, and examples/LogisticRegression through the tensor plane at W = 1.

``reference`` is plain float64 numpy on the fp32 inputs; given a result it asserts
the contract of ops/glm.py's docstring for every cell.
"""
import numpy as np
import pytest
import torch

LR = "lua_mapreduce_1_amd.examples.LogisticRegression"


def reference(X, y, beta, got=None, bounds=None, exact=False):
    Z = np.column_stack([X, np.ones(len(X))]).astype(np.float64)
    eta = Z @ beta.astype(np.float64)
    mu = 0.5 * (1 + np.tanh(0.5 * eta))  # not the kernel's formula
    ll64 = float((y * eta - np.logaddexp(0.0, eta)).sum())
    g64, H64 = Z.T @ (y - mu), (Z * (mu * (1 - mu))[:, None]).T @ Z
    if got is None:
        return ll64, g64, H64
    ll, g, H = (t.cpu().numpy() for t in got)
    assert ll.dtype == g.dtype == H.dtype == np.float64 and ll.shape == (1,) and g.shape == g64.shape \
        and H.shape == H64.shape
    assert np.isfinite(ll).all() and np.isfinite(g).all() and np.isfinite(H).all()
    assert np.array_equal(H, H.T) and (np.diag(H) >= 0).all()
    if exact:
        assert np.array_equal(g, g64) and np.array_equal(H, H64)
    if bounds is not None:
        bl, bg, bH = (t.cpu().numpy() for t in bounds)
        shares = [float((np.abs(a - b) / np.maximum(c, 1e-300)).max())
                  for a, b, c in ((ll, ll64, bl), (g, g64, bg), (H, H64, bH))]
        print("worst error / bound (ll, g, H)", shares)
        assert max(shares) <= 1
    return ll64, g64, H64


def small_ints(n, d):
    """X in -15..15, y in {0, 1}, beta = 0: every fp32 operation on g and H is exact."""
    rng = np.random.default_rng(n + d)
    return (rng.integers(-15, 16, (n, d)).astype(np.float32), rng.integers(0, 2, n).astype(np.float32),
            np.zeros(d + 1, dtype=np.float32))


def normal(n, d):
    """Unit normals, an asymmetric beta ~ N(0, 1 / d), and four rows scaled to eta ~ +-200 (saturation)."""
    rng = np.random.default_rng(n + d)
    X = rng.standard_normal((n, d)).astype(np.float32)
    beta = (rng.standard_normal(d + 1) / np.sqrt(d)).astype(np.float32)
    b = beta[:d].astype(np.float64)
    X[:4] = (np.array([200.0, -200.0, 150.0, -250.0])[:, None] * b / (b @ b)).astype(np.float32)
    return X, rng.integers(0, 2, n).astype(np.float32), beta


def tens(*arrays, device="cpu"):
    return tuple(torch.from_numpy(a).to(device) for a in arrays)


@pytest.mark.parametrize("n,d", [(0, 4), (3, 5), (70, 16), (300, 127)])
def test_cpu_specification(n, d):
    from lua_mapreduce_1_amd.ops import glm as Gl
    for make in (small_ints, normal):
        if make is normal and n < 4:
            continue
        X, y, beta = make(n, d)
        tx, ty, tb = tens(X, y, beta)
        reference(X, y, beta, Gl.newton_stats(tx, ty, tb), bounds=Gl.error_terms(tx, ty, tb, 1), exact=make is small_ints)
    ll, g, H = Gl.newton_stats(tx[:n // 2].contiguous(), ty[:n // 2].contiguous(), tb)
    got = Gl.newton_stats(tx[n // 2:].contiguous(), ty[n // 2:].contiguous(), tb, ll=ll, g=g, H=H)
    assert got[0] is ll and got[1] is g and got[2] is H
    reference(X, y, beta, got, bounds=Gl.error_terms(tx, ty, tb, 1))


def problem(n=600, d=5, seed=11):
    from lua_mapreduce_1_amd.examples import LogisticRegression as m
    return m.make_problem(seed, n, d, 3)


@pytest.mark.parametrize("l2", [0.0, 3.0])
def test_newton_step_and_fit(l2):
    from lua_mapreduce_1_amd.examples import LogisticRegression as m
    from lua_mapreduce_1_amd.ops import glm as Gl
    splits = problem()
    R = np.concatenate(splits)
    tx, ty = tens(np.ascontiguousarray(R[:, :-1]), np.ascontiguousarray(R[:, -1]))
    want = m.naive(splits, l2=l2)
    beta, history = Gl.fit(tx, ty, l2=l2)
    assert beta.dtype == torch.float32 and np.allclose(beta.numpy(), want["beta"], rtol=0, atol=1e-6)
    assert history[0]["iter"] == 0 and abs(history[-1]["ll"] - want["history"][-1]["ll"]) <= 1e-6
    assert all(h["halvings"] == 0 for h in history) and history[1]["ll"] > history[0]["ll"]
    # one step from zero against a dense numpy solve
    b0 = torch.zeros(6)
    delta = Gl.newton_step(b0, *Gl.newton_stats(tx, ty, b0), l2=l2).numpy()
    _ll, g64, H64 = reference(R[:, :-1], R[:, -1], np.zeros(6))
    pen = np.diag([1.0] * 5 + [0.0])
    assert np.allclose(delta, np.linalg.solve(H64 + l2 * pen, g64), rtol=1e-10)
    assert np.allclose(Gl.predict_proba(tx, beta).numpy(), 1 / (1 + np.exp(-(R[:, :-1] @ beta.numpy()[:-1] + beta.numpy()[-1]))),
                       atol=1e-6)


@pytest.mark.parametrize("edit,exc", [
    (lambda a: dict(a, X=torch.zeros(9, 128), beta=torch.zeros(129)), ValueError),
    (lambda a: dict(a, X=a["X"].double()), TypeError),
    (lambda a: dict(a, X=torch.zeros(8, 9).t()), ValueError),
    (lambda a: dict(a, y=torch.zeros(8)), ValueError),
    (lambda a: dict(a, beta=torch.zeros(8)), ValueError),
    (lambda a: dict(a, H=torch.zeros(9, 9)), ValueError),
    (lambda a: dict(a, slabs=0), ValueError),
], ids=["d128", "fp64", "strided", "y-len", "beta-len", "H-dtype", "slabs0"])
def test_argument_checks(edit, exc):
    from lua_mapreduce_1_amd.ops import glm as Gl
    with pytest.raises(exc):
        Gl.newton_stats(**edit(dict(X=torch.zeros(9, 8), y=torch.zeros(9), beta=torch.zeros(9))))


def run_job(device, splits, args):
    """Run examples/LogisticRegression and hold its result to ``naive``."""
    import importlib
    from lua_mapreduce_1_amd import spmd
    from lua_mapreduce_1_amd.ops import glm as Gl
    m = importlib.import_module(LR)
    tol = 1e-6
    eng = spmd(dict(taskfn=LR, mapfn=LR, partitionfn=LR, reducefn=LR, finalfn=LR, init_args={**args, "tol": tol}),
               device=device)
    assert eng.plane_kind == "tensor"
    res = eng.run()
    R = np.concatenate(splits)
    assert int(m._km.rejoin_counts(res.tensors["ROWS"])[0]) == len(R)
    want = m.naive(splits, l2=args.get("l2", 0.0), tol=tol)
    # The job stops where its own gradient vanishes, so the true gradient there is minus the error dg of the
    # last pass, |dg_c| <= bg_c by the contract (error_terms), and BETA - beta* = (H + l2 I')^-1 dg to first order:
    # at most |bg|_2 / lambda_min in any coordinate.  Both sides stop after a move <= tol of a quadratically
    # convergent iteration (what is left is far below tol: 2 tol covers both), and BETA is the fp32 rounding of
    # the float64 iterate (u |beta|).  The factor 2 on the first term covers the second order and the error of H.
    tx, ty, tb = tens(np.ascontiguousarray(R[:, :-1]), np.ascontiguousarray(R[:, -1]), want["beta"].astype(np.float32))
    _bl, bg, _bH = Gl.error_terms(tx, ty, tb, Gl.MAX_SLABS)
    H64 = reference(R[:, :-1], R[:, -1], want["beta"])[2] + args.get("l2", 0.0) * np.diag([1.0] * (R.shape[1] - 1) + [0.0])
    lam = np.linalg.eigvalsh(H64)[0]
    bound = 2 * float(np.linalg.norm(bg.numpy())) / lam + 2 * tol + 2.0 ** -24 * np.abs(want["beta"])
    err = np.abs(m.BETA.cpu().numpy() - want["beta"])
    print("lambda_min", lam, "worst |BETA - naive| / tolerance", (err / bound).max(), "passes", len(m.HISTORY))
    assert (err <= bound).all()
    assert m.HISTORY[0]["iter"] == 0 and abs(m.HISTORY[-1]["ll"] - want["history"][-1]["ll"]) <= 1e-6 * len(R)
    pr = m.predict(R[:100, :-1]).cpu().numpy()
    assert np.allclose(pr, 1 / (1 + np.exp(-(R[:100, :-1] @ want["beta"][:-1] + want["beta"][-1]))), atol=1e-4)
    return m


def test_job_cpu_w1_against_naive(tmp_path):
    splits = problem(3000, 6, 3)
    files = []
    for i, s in enumerate(splits):
        files.append(str(tmp_path / f"rows{i}.f32"))
        s.astype("<f4").tofile(files[-1])
    m = run_job(torch.device("cpu"), splits, {"files": files, "dim": 6, "l2": 0.5})
    assert m.BETA.shape == (7,) and m.BETA.dtype == torch.float32
    with pytest.raises(RuntimeError):
        m.mapfn(None, None, None)
