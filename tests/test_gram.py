"""ops.gram on CPU tensors (the executable specification), its float64 helpers,
the argument checks, and examples/PCA through the tensor plane at W = 1.

``reference`` is plain float64 numpy on ``zc = fl32(z - shift)``; given a result
it asserts the contract of ops/gram.py's docstring for every cell.
"""
import numpy as np
import pytest
import torch

PC = "lua_mapreduce_1_amd.examples.PCA"


def reference(X, Y, shift, got=None, factor=None, exact=False):
    Z = X if Y is None else np.concatenate([X, Y], axis=1)
    zc = (Z if shift is None else Z - shift).astype(np.float64)  # Z - shift is the fp32 subtraction
    s64, G64 = zc.sum(0), zc.T @ zc
    if got is None:
        return s64, G64
    s, G = (t.cpu().numpy() for t in got)
    assert s.dtype == G.dtype == np.float64 and s.shape == s64.shape and G.shape == G64.shape
    assert np.array_equal(G, G.T) and (np.diag(G) >= 0).all()
    if exact:
        assert np.array_equal(s, s64) and np.array_equal(G, G64)
    if factor is not None:
        a = np.abs(zc)
        share = max((np.abs(G - G64) / np.maximum(factor * (a.T @ a), 1e-300)).max(initial=0.0),
                    (np.abs(s - s64) / np.maximum(factor * a.sum(0), 1e-300)).max(initial=0.0))
        print("worst error / bound", share)
        assert share <= 1
    return s64, G64


def small_ints(n, d, t, shift=False):
    """Shifted values in -15..15: a run's sums stay below 2^24, every fp32 operation is exact."""
    rng = np.random.default_rng(n + d + t)
    sh = rng.integers(-40, 41, d + t).astype(np.float32) if shift else None
    Z = rng.integers(-15, 16, (n, d + t)).astype(np.float32) + (sh if shift else 0)
    return np.ascontiguousarray(Z[:, :d]), (np.ascontiguousarray(Z[:, d:]) if t else None), sh


def normal(n, d, t, shift=False):
    """Unit normals around a common offset of about 100, so the shift matters."""
    rng = np.random.default_rng(n + d + t)
    Z = (100.0 + rng.standard_normal((n, d + t))).astype(np.float32)
    sh = Z[:64].astype(np.float64).mean(0).astype(np.float32) if shift else None
    return np.ascontiguousarray(Z[:, :d]), (np.ascontiguousarray(Z[:, d:]) if t else None), sh


def tens(*arrays, device="cpu"):
    return tuple(None if a is None else torch.from_numpy(a).to(device) for a in arrays)


@pytest.mark.parametrize("n,d,t,shift", [(0, 4, 0, False), (3, 5, 0, True), (70, 17, 2, True), (300, 129, 0, False)])
def test_cpu_specification(n, d, t, shift):
    from lua_mapreduce_1_amd.ops import gram as Gm
    for make in (small_ints, normal):
        X, Y, sh = make(n, d, t, shift)
        tx, ty, ts = tens(X, Y, sh)
        reference(X, Y, sh, Gm.moments(tx, ty, ts), factor=Gm.error_factor(n, 1), exact=make is small_ints)
    s, G = Gm.moments(tx[:n // 2].contiguous(), None if ty is None else ty[:n // 2].contiguous(), ts)
    s2, G2 = Gm.moments(tx[n // 2:].contiguous(), None if ty is None else ty[n // 2:].contiguous(), ts, s=s, G=G)
    assert s2 is s and G2 is G
    reference(X, Y, sh, (s, G), factor=Gm.error_factor(n, 1))


def test_covariance_pca_ridge():
    from lua_mapreduce_1_amd.ops import gram as Gm
    rng = np.random.default_rng(7)
    X = (rng.standard_normal((500, 6)) * np.array([5, 4, 3, 2, 1, 0.5]) + 50).astype(np.float32)
    Y = (X.astype(np.float64) @ rng.standard_normal((6, 2)) + 3 + 0.01 * rng.standard_normal((500, 2))).astype(np.float32)
    sh = np.concatenate([X, Y], 1)[:32].mean(0).astype(np.float32)
    Z = np.concatenate([X, Y], 1).astype(np.float64)
    for shift in (None, sh):
        s, G = Gm.moments(*tens(X, Y, shift))
        cov = Gm.covariance(500, s, G).numpy()
        assert np.allclose(cov, np.cov(Z, rowvar=False), rtol=0, atol=1e-9 * np.abs(cov).max() * (1 if shift is not None else 1e4))
        comp, var, off = Gm.pca(500, s, G, 3)
        val, vec = np.linalg.eigh(np.cov(Z, rowvar=False))
        assert np.allclose(var.numpy(), val[::-1][:3], rtol=1e-7)
        assert np.allclose(np.abs(comp.numpy() @ vec[:, ::-1][:, :3]), np.eye(3), atol=1e-6)
        assert (comp.numpy()[np.arange(3), np.abs(comp.numpy()).argmax(1)] > 0).all()
        assert np.allclose(off.numpy() + (0 if shift is None else shift), Z.mean(0), rtol=1e-9)
        coef, icpt = Gm.ridge(500, s, G, 6, shift=None if shift is None else torch.from_numpy(shift))
        want = np.linalg.lstsq(np.concatenate([Z[:, :6], np.ones((500, 1))], 1), Z[:, 6:], rcond=None)[0]
        assert np.allclose(coef.numpy(), want[:6], atol=1e-6) and np.allclose(icpt.numpy(), want[6], atol=1e-4)
    lam = Gm.ridge(500, s, G, 6, lam=1e6)[0]
    assert float(lam.abs().max()) < float(coef.abs().max())


@pytest.mark.parametrize("edit,exc", [
    (lambda a: dict(a, X=torch.zeros(9, 257)), ValueError),
    (lambda a: dict(a, X=torch.zeros(9, 250), Y=torch.zeros(9, 7)), ValueError),
    (lambda a: dict(a, X=a["X"].double()), TypeError),
    (lambda a: dict(a, X=torch.zeros(8, 9).t()), ValueError),
    (lambda a: dict(a, Y=torch.zeros(8, 2)), ValueError),
    (lambda a: dict(a, shift=torch.zeros(7)), ValueError),
    (lambda a: dict(a, G=torch.zeros(8, 8)), ValueError),
    (lambda a: dict(a, slabs=0), ValueError),
], ids=["w257", "d+t257", "fp64", "strided", "Y-rows", "shift-len", "G-dtype", "slabs0"])
def test_argument_checks(edit, exc):
    from lua_mapreduce_1_amd.ops import gram as Gm
    with pytest.raises(exc):
        Gm.moments(**edit(dict(X=torch.zeros(9, 8))))


def run_job(device, splits, args, components):
    """Run examples/PCA and hold its result to ``naive``."""
    import importlib
    from lua_mapreduce_1_amd import spmd
    from lua_mapreduce_1_amd.ops import gram as Gm
    m = importlib.import_module(PC)
    eng = spmd(dict(taskfn=PC, mapfn=PC, partitionfn=PC, reducefn=PC, finalfn=PC,
                    init_args={**args, "components": components}), device=device)
    assert eng.plane_kind == "tensor"
    res = eng.run()
    n = sum(len(s) for s in splits)
    assert int(m._km.rejoin_counts(res.tensors["ROWS"])[0]) == n
    mean, comp, var, cov = m.naive(splits, components)
    # covariance = (G - s s^T / n) / (n - 1) of the shifted rows.  With f the contract's factor and
    # q_i = sqrt(sum zc_i^2): |dG_ij| <= f sum |zc_i zc_j| <= f q_i q_j (Cauchy-Schwarz), and |d(s_i s_j / n)|
    # <= 2 f (sum |zc_i|)(sum |zc_j|) / n <= 2 f q_i q_j: 3 f q_i q_j / (n - 1), plus the oracle's own float64 noise
    zc = np.concatenate(splits).astype(np.float64) - m._st["shift"]
    scale = np.sqrt((zc * zc).sum(0))
    tol = 3 * Gm.error_factor(n, Gm.MAX_SLABS) * np.outer(scale, scale) / (n - 1) + 1e-12 * np.abs(cov).max()
    assert (np.abs(m.COVARIANCE.cpu().numpy() - cov) <= tol).all()
    # the blobs of make_points have centres N(0, 10^2) and unit spread: the leading eigenvalues are of the
    # order of 100 and differ by more than 10 % of the largest (asserted), so an eigenvector moves by about
    # |dC| / gap ~ 1e-5: well inside 1e-4 in absolute cosine
    assert (np.diff(-var) > 0.1 * var[0]).all()
    cos = np.abs((m.COMPONENTS.cpu().numpy() * comp).sum(1))
    print("eigen-gaps", np.diff(-var), "1 - |cos|", 1 - cos)
    assert (cos >= 1 - 1e-4).all()
    assert np.allclose(m.EXPLAINED_VARIANCE.cpu().numpy(), var, rtol=1e-4)
    assert np.allclose(m.MEAN.cpu().numpy(), mean, rtol=0, atol=1e-4)
    return m


def test_job_cpu_w1_against_naive(tmp_path):
    from lua_mapreduce_1_amd.examples import KMeans as km
    splits = km.make_points(3, 3000, 6, 5, 3)
    files = []
    for i, s in enumerate(splits):
        files.append(str(tmp_path / f"points{i}.f32"))
        s.astype("<f4").tofile(files[-1])
    m = run_job(torch.device("cpu"), splits, {"files": files, "dim": 6}, 3)
    assert m.COMPONENTS.shape == (3, 6) and m.COVARIANCE.shape == (6, 6)
    with pytest.raises(RuntimeError):
        m.mapfn(None, None, None)
