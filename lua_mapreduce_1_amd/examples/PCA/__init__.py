"""Principal component analysis as a MapReduce job on the tensor plane.

One module provides every function (pass it as taskfn, mapfn, partitionfn,
reducefn and finalfn) and runs in SPMD form only, like examples/KNN; it reuses
examples/KMeans' point files, synthetic points and row access.  A split's
statistics are a small matrix and the reduce is a sum.

* ``init(args)``: ``files`` — raw little-endian fp32 ``[n_i, dim]`` row-major
  files, one per map job, or ``"synthetic"`` (``examples.KMeans.make_points(seed,
  n, dim, blobs, nsplits)``) — ``dim``, ``components``, ``seed``.  The shift is the
  float64 mean of the first min(4096, n_0) rows of split 0, rounded to fp32,
  computed once and replicated (ops/gram.py says why a rough mean is enough).
* map: one job per file.  The job's points go to the device once and
  ``ops.gram.moments`` (csrc/hip/gram.hip) folds them into the rank's running
  float64 ``(s, G)``; the number of rows is ADDED into the plane's one key,
  ``ROWS`` (as two exact fp32 words, like KMeans' counts).
* final (every rank): checks that ``ROWS`` is the size of the data set, gathers
  the ranks' ``(s, G)`` (``parallel.dist.all_gather_tensor``) and adds them in
  rank order in float64 — the statistics never pass through the plane's fp32
  sum.  ``MEAN`` [dim], ``COMPONENTS`` [components, dim], ``EXPLAINED_VARIANCE``
  [components] and ``COVARIANCE`` [dim, dim] (float64) stay on the device.  One
  iteration, no loop.
* ``naive(splits, components)``: the float64 numpy oracle (``np.cov`` and
  ``eigh``, the same sign rule).
"""
from __future__ import annotations

import numpy as np
import torch

from lua_mapreduce_1_amd.examples import KMeans as _km
from lua_mapreduce_1_amd.ops import gram as Gm
from lua_mapreduce_1_amd.ops import io as _io
from lua_mapreduce_1_amd.parallel import dist as D

NUM_REDUCERS = 10
SHIFT_ROWS = 4096

device_reduce = "tensor_sum"
spmd_replicated_taskfn = True

MEAN = COMPONENTS = EXPLAINED_VARIANCE = COVARIANCE = None
_st: dict = {}


def init(args):
    global MEAN, COMPONENTS, EXPLAINED_VARIANCE, COVARIANCE
    a = dict(args or {})
    _st.clear()
    MEAN = COMPONENTS = EXPLAINED_VARIANCE = COVARIANCE = None
    dim, seed = int(a["dim"]), int(a.get("seed", 0))
    files = a.get("files", "synthetic")
    if files == "synthetic":
        splits = _km.make_points(seed, int(a.get("n", 20000)), dim, int(a.get("blobs", 8)), int(a.get("nsplits", 4)))
    else:
        splits = [files] if isinstance(files, str) else list(files)
    head = np.asarray(_km._rows(splits[0], dim)[:SHIFT_ROWS], dtype=np.float64)
    shift = (head.mean(0) if len(head) else np.zeros(dim)).astype(np.float32)
    _st.update(dim=dim, components=int(a.get("components", dim)), splits=splits, shift=shift,
               total=int(sum(_km._rows(s, dim).shape[0] for s in splits)), stats=None)


def taskfn(emit):
    for j, s in enumerate(_st["splits"]):
        emit(j + 1, j if isinstance(s, np.ndarray) else s)


def device_tensor_layout() -> dict:
    return {"ROWS": 2}


def _points(value, device) -> torch.Tensor:
    if isinstance(value, str):
        return _io.load_file(value, device).view(torch.float32).view(-1, _st["dim"])
    return torch.from_numpy(_st["splits"][int(value)]).to(device)


def _stats(device):
    """The replicated shift and this rank's running (s, G), on the device."""
    if _st["stats"] is None:
        shift = torch.from_numpy(_st["shift"]).to(device)
        _st["stats"] = (shift,) + Gm.moments(torch.empty((0, _st["dim"]), dtype=torch.float32, device=device))
    return _st["stats"]


def device_mapfn(key, value, emit):
    """Fold the job's split into the rank's running moments."""
    x = _points(value, emit.device)
    shift, s, G = _stats(emit.device)
    Gm.moments(x, shift=shift, s=s, G=G)
    rows = emit.accumulator("ROWS")
    seen = _km.rejoin_counts(rows) + x.shape[0]
    rows.copy_(_km.split_counts(seen))


def partitionfn(key):
    return sum(key.encode()) % NUM_REDUCERS


def reducefn(key, values, emit):
    emit(sum(np.asarray(v, dtype=np.float64) for v in values))


def device_finalfn(res, engine):
    """Every rank: all rows seen?  Then add the ranks' moments in rank order and decompose."""
    global MEAN, COMPONENTS, EXPLAINED_VARIANCE, COVARIANCE
    n = int(_km.rejoin_counts(res.tensors["ROWS"])[0])
    if n != _st["total"]:
        raise RuntimeError(f"examples/PCA: {n} rows were folded, the splits hold {_st['total']}")
    shift, s, G = _stats(engine.device)
    w = s.shape[0]
    both = D.all_gather_tensor(torch.cat([s[None], G]), engine.group).view(-1, w + 1, w)
    tot = both[0].clone()
    for r in range(1, both.shape[0]):  # float64, in rank order
        tot += both[r]
    s, G = tot[0], tot[1:]
    COMPONENTS, EXPLAINED_VARIANCE, off = Gm.pca(n, s, G, _st["components"])
    MEAN, COVARIANCE = off + shift.double(), Gm.covariance(n, s, G)
    return True


def finalfn(pairs):
    raise RuntimeError("examples/PCA runs in SPMD form only (device_finalfn)")


def mapfn(key, value, emit):
    raise RuntimeError("examples/PCA runs in SPMD form only (device_mapfn)")


def naive(splits, components: int):
    """``(mean, components, explained_variance, covariance)`` in plain float64 numpy."""
    X = np.concatenate([np.asarray(s) for s in splits]).astype(np.float64)
    cov = np.atleast_2d(np.cov(X, rowvar=False))
    val, vec = np.linalg.eigh(cov)
    comp = vec[:, ::-1].T[:components]
    big = comp[np.arange(len(comp)), np.abs(comp).argmax(1)]
    return X.mean(0), comp * np.where(big < 0, -1.0, 1.0)[:, None], val[::-1][:components], cov
