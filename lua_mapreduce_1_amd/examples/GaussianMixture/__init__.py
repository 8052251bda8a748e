"""A diagonal-covariance Gaussian mixture fitted by EM, as an iterative
MapReduce job on the tensor plane.

One module provides every function (pass it as taskfn, mapfn, partitionfn,
reducefn and finalfn) and runs in SPMD form only, like examples/KMeans, whose
point files, synthetic points and row picking it reuses.

* ``init(args)``: ``files`` — raw little-endian fp32 ``[n_i, dim]`` row-major
  files, one per map job, or ``"synthetic"`` (``examples.KMeans.make_points(seed,
  n, dim, k, nsplits)``) — ``k``, ``dim``, ``max_iters`` (50), ``tol`` (1e-5),
  ``reg_covar`` (1e-6), ``seed``, and optionally ``means`` (array or raw fp32
  file).  Without ``means`` every rank picks the same k distinct rows exactly as
  KMeans' ``"rows"`` does.  The initial variances are the global per-coordinate
  variance of the points (float64 on the host, one pass), the weights uniform.
* map: one job per file.  The job's points go to the device once and stay
  there; ``ops.gmm.estep`` (csrc/hip/gmm.hip: three launches, both matrix
  products on the fp32 matrix cores) runs against the replicated parameters and
  its float64 statistics are ADDED into the plane as fp32: ``NK`` [k], ``S1``
  [k*dim], ``S2`` [k*dim], ``LL`` [1].
* final (every rank), in float64: ``HISTORY`` gets ``{iter, ll, change}`` with
  ``ll`` the log-likelihood of the parameters the iteration STARTED from.  The
  job stops when ``|change| <= tol |ll|`` or at ``max_iters``; the stopping
  iteration only evaluates, so the last ``ll`` is the log-likelihood of the
  model that is returned.  Otherwise the M-step follows: ``w = nk / sum nk``,
  ``mu = s1 / nk``, ``var = max(s2 / nk - mu^2, 0) + reg_covar``; a component
  with ``nk < 10 u n`` (u = 2^-24) keeps its parameters.  They are stored back
  as fp32 and the job returns ``"loop"``.
* afterwards ``WEIGHTS`` / ``MEANS`` / ``VARIANCES`` are device tensors and
  ``predict(X)`` / ``score_samples(X)`` serve the model.
* ``naive(splits, ...)``: the same EM in float64 numpy with the same init,
  floor, keep rule and stopping rule.
"""
from __future__ import annotations

import numpy as np
import torch

from lua_mapreduce_1_amd.examples import KMeans as _km
from lua_mapreduce_1_amd.ops import gmm as G
from lua_mapreduce_1_amd.ops import io as _io

NUM_REDUCERS = 10
U = 2.0 ** -24

device_reduce = "tensor_sum"
spmd_replicated_taskfn = True

HISTORY: list = []
WEIGHTS = MEANS = VARIANCES = None
_st: dict = {}


def global_variance(splits, dim: int) -> np.ndarray:
    """Per-coordinate variance of the concatenated splits, float64."""
    n, s, q = 0, np.zeros(dim), np.zeros(dim)
    for sp in splits:
        x = np.asarray(_km._rows(sp, dim), dtype=np.float64)
        n, s, q = n + len(x), s + x.sum(0), q + (x * x).sum(0)
    return np.maximum(q / n - (s / n) ** 2, 0.0)


def initial_parameters(splits, k: int, dim: int, seed: int, reg_covar: float, means=None):
    """``(weights [k], means [k, dim], variances [k, dim])`` fp32, the same on every rank."""
    if means is None:
        m0 = _km.initial_centroids(splits, k, dim, seed)
    elif isinstance(means, str):
        m0 = np.fromfile(means, dtype="<f4").reshape(k, dim)
    else:
        m0 = np.asarray(means, dtype=np.float32).reshape(k, dim)
    v0 = np.tile(global_variance(splits, dim) + reg_covar, (k, 1))
    return (np.full(k, 1.0 / k, dtype=np.float32), np.ascontiguousarray(m0, dtype=np.float32),
            np.ascontiguousarray(v0, dtype=np.float32))


def init(args):
    global HISTORY, WEIGHTS, MEANS, VARIANCES
    a = dict(args or {})
    _st.clear()
    HISTORY = []
    WEIGHTS = MEANS = VARIANCES = None
    k, dim, seed = int(a["k"]), int(a["dim"]), int(a.get("seed", 0))
    files = a.get("files", "synthetic")
    if files == "synthetic":
        splits = _km.make_points(seed, int(a.get("n", 20000)), dim, k, int(a.get("nsplits", 4)))
    else:
        splits = [files] if isinstance(files, str) else list(files)
    reg = float(a.get("reg_covar", 1e-6))
    _st.update(k=k, dim=dim, splits=splits, points={}, reg=reg, max_iters=int(a.get("max_iters", 50)),
               tol=float(a.get("tol", 1e-5)), p0=initial_parameters(splits, k, dim, seed, reg, a.get("means")))


def taskfn(emit):
    for j, s in enumerate(_st["splits"]):
        emit(j + 1, j if isinstance(s, np.ndarray) else s)


def device_tensor_layout() -> dict:
    return {"NK": _st["k"], "S1": _st["k"] * _st["dim"], "S2": _st["k"] * _st["dim"], "LL": 1}


def _params(device):
    global WEIGHTS, MEANS, VARIANCES
    if MEANS is None:
        WEIGHTS, MEANS, VARIANCES = (torch.from_numpy(p).to(device) for p in _st["p0"])
    return WEIGHTS, MEANS, VARIANCES


def _points(key, value, device) -> torch.Tensor:
    x = _st["points"].get(key)
    if x is None:
        if isinstance(value, str):
            x = _io.load_file(value, device).view(torch.float32).view(-1, _st["dim"])
        else:
            x = torch.from_numpy(_st["splits"][int(value)]).to(device)
        _st["points"][key] = x
    return x


def device_mapfn(key, value, emit):
    """One E-step over the job's resident points; its statistics are added into the plane."""
    dev = emit.device
    nk, s1, s2, ll, _logp, _lab = G.estep(_points(key, value, dev), *_params(dev))
    emit.accumulator("NK").add_(nk.to(torch.float32))
    emit.accumulator("S1").add_(s1.reshape(-1).to(torch.float32))
    emit.accumulator("S2").add_(s2.reshape(-1).to(torch.float32))
    emit.accumulator("LL").add_(ll.to(torch.float32))


def partitionfn(key):
    return sum(key.encode()) % NUM_REDUCERS


def reducefn(key, values, emit):
    emit(sum(np.asarray(v, dtype=np.float64) for v in values))


def m_step(nk, s1, s2, w, mu, var, reg):
    """The M-step on float64 arrays or tensors ([k], [k, d], [k, d]; the old
    parameters likewise): a component below 10 u n keeps what it had."""
    where, zero = (torch.where, torch.zeros_like) if isinstance(nk, torch.Tensor) else (np.where, np.zeros_like)
    n = nk.sum()
    live = nk >= 10 * U * n
    safe = where(live, nk, zero(nk) + 1)[:, None]
    m = s1 / safe
    v = s2 / safe - m * m
    v = where(v > 0, v, zero(v)) + reg
    return where(live, nk / n, w), where(live[:, None], m, mu), where(live[:, None], v, var)


def device_finalfn(res, engine):
    """Every rank: record the log-likelihood, stop or take the M-step."""
    global WEIGHTS, MEANS, VARIANCES
    k, dim = _st["k"], _st["dim"]
    ll = float(res.tensors["LL"][0])
    change = ll - HISTORY[-1]["ll"] if HISTORY else float("inf")
    HISTORY.append({"iter": len(HISTORY) + 1, "ll": ll, "change": change})
    if engine.rank == 0 and engine.verbose:
        print("# gmm iter %(iter)d ll %(ll).8g change %(change).3g" % HISTORY[-1], flush=True)
    if abs(change) <= _st["tol"] * abs(ll) or len(HISTORY) >= _st["max_iters"]:
        return True
    w, mu, var = (p.to(torch.float64) for p in _params(engine.device))
    t = res.tensors
    w, mu, var = m_step(t["NK"].to(torch.float64), t["S1"].view(k, dim).to(torch.float64),
                        t["S2"].view(k, dim).to(torch.float64), w, mu, var, _st["reg"])
    WEIGHTS, MEANS, VARIANCES = (p.to(torch.float32).contiguous() for p in (w, mu, var))
    return "loop"


def finalfn(pairs):
    raise RuntimeError("examples/GaussianMixture runs in SPMD form only (device_finalfn)")


def mapfn(key, value, emit):
    raise RuntimeError("examples/GaussianMixture runs in SPMD form only (device_mapfn)")


def _rows_on_device(X) -> torch.Tensor:
    x = torch.from_numpy(np.ascontiguousarray(X, dtype=np.float32)) if isinstance(X, np.ndarray) else torch.as_tensor(X)
    return x.to(torch.float32).to(MEANS.device).contiguous()


def predict(X) -> torch.Tensor:
    """int32 arg-max component of the rows of X under the fitted mixture."""
    return G.predict(_rows_on_device(X), WEIGHTS, MEANS, VARIANCES)


def score_samples(X) -> torch.Tensor:
    """fp32 log-density of the rows of X under the fitted mixture."""
    return G.score_samples(_rows_on_device(X), WEIGHTS, MEANS, VARIANCES)


def log_density(X, w, mu, var):
    """float64 numpy ``(S [n, k], logp [n])`` of the plain formula, in row blocks."""
    X, w, mu, var = (np.asarray(t, dtype=np.float64) for t in (X, w, mu, var))
    S = np.empty((len(X), len(w)))
    const = np.log(w) - 0.5 * np.log(2 * np.pi * var).sum(1)
    rows = max(1, (1 << 22) // mu.size)
    for i in range(0, len(X), rows):
        S[i:i + rows] = const - 0.5 * (((X[i:i + rows, None, :] - mu[None]) ** 2) / var[None]).sum(-1)
    m = S.max(1)
    return S, m + np.log(np.exp(S - m[:, None]).sum(1))


def naive(splits, k: int, dim: int, max_iters: int = 50, tol: float = 1e-5, seed: int = 0, means=None,
          reg_covar: float = 1e-6) -> dict:
    """Plain float64 numpy EM: the oracle of the job above."""
    X = np.concatenate([np.asarray(_km._rows(s, dim)) for s in splits]).astype(np.float64)
    w, mu, var = (p.astype(np.float64) for p in initial_parameters(splits, k, dim, seed, reg_covar, means))
    history = []
    while True:
        S, logp = log_density(X, w, mu, var)
        ll = float(logp.sum())
        change = ll - history[-1]["ll"] if history else float("inf")
        history.append({"iter": len(history) + 1, "ll": ll, "change": change})
        if abs(change) <= tol * abs(ll) or len(history) >= max_iters:
            return {"weights": w, "means": mu, "variances": var, "history": history}
        R = np.exp(S - logp[:, None])
        w, mu, var = m_step(R.sum(0), R.T @ X, R.T @ (X * X), w, mu, var, reg_covar)
