"""The map step of Lloyd's k-means: nearest-centroid assignment and the
per-cluster partial sums in ONE launch (csrc/hip/kmeans.hip: distances on the
fp32 matrix cores, argmin in registers, sums combined in LDS; the n x k
distance matrix never exists).

``step(X, C)`` assigns every row of ``X`` [n, d] to its nearest row of ``C``
[k, d] and adds, into float64 ``sums`` [k, d], int64 ``counts`` [k] and float64
``cost`` [1], the members' coordinate sums, their number and the sum of squared
distances.  ``assign(X, C)`` is the labels-only mode of the same kernel.

Supported: contiguous fp32 ``X`` and ``C`` on one device, 1 <= d <= 512,
1 <= k <= 4096, n >= 0.  Anything else raises; on a GPU there is no torch
fallback.  CPU tensors run the executable specification below (float64
distances, first minimum, ``index_add_``).

Numeric contract (u = 2^-24, gamma_m = m u / (1 - m u)):

* labels: the kernel minimises the fp32 score ``|c_j|^2 - 2 x.c_j`` (two
  length-d fma chains and one subtract), so the chosen centroid is within
  ``E_i = 2 gamma_{d+2} (|x_i| + max_j |c_j|)^2`` of the float64 minimum
  squared distance, and IS the float64 argmin wherever the float64 margin
  exceeds ``E_i``.  Ties (equal fp32 scores; identical centroids always tie)
  go to the lowest centroid index, deterministically.
* counts are exact and consistent with the labels.
* sums: the members' coordinates added in any order, partly in fp32:
  ``|sums[j, c] - exact| <= 2 gamma_{n_j} sum_members |x_c|`` (the contract of
  the typed folds, ops/agg.py).
* cost: ``sum_i max(0, |x_i|^2 + score_i)``; within
  ``sum_i (E_i + gamma_{d+2} |x_i|^2) + gamma_n cost`` of the float64 cost.
* non-finite coordinates: unspecified (labels stay inside [0, k)).
"""
from __future__ import annotations

import torch

MAX_D = 512
MAX_K = 4096


def _check(X: torch.Tensor, C: torch.Tensor) -> tuple[int, int, int]:
    for name, t in (("X", X), ("C", C)):
        if not isinstance(t, torch.Tensor):
            raise TypeError(f"kmeans: {name} must be a torch tensor (got {type(t).__name__})")
        if t.dtype != torch.float32:
            raise TypeError(f"kmeans: {name} must be float32 (got {t.dtype})")
        if t.dim() != 2:
            raise ValueError(f"kmeans: {name} must be 2-D [rows, d] (got {tuple(t.shape)})")
        if not t.is_contiguous():
            raise ValueError(f"kmeans: {name} must be contiguous")
    if X.device != C.device:
        raise ValueError(f"kmeans: X is on {X.device}, C on {C.device}")
    n, d = X.shape
    k = C.shape[0]
    if C.shape[1] != d:
        raise ValueError(f"kmeans: X has d = {d}, C has d = {C.shape[1]}")
    if not 1 <= d <= MAX_D:
        raise ValueError(f"kmeans: d = {d} is outside 1..{MAX_D}")
    if not 1 <= k <= MAX_K:
        raise ValueError(f"kmeans: k = {k} is outside 1..{MAX_K}")
    return n, d, k


def _acc(t, shape, dtype, device, name):
    if t is None:
        return torch.zeros(shape, dtype=dtype, device=device)
    if t.dtype != dtype or tuple(t.shape) != tuple(shape) or t.device != device or not t.is_contiguous():
        raise ValueError(f"kmeans: {name} must be a contiguous {dtype} tensor of shape {tuple(shape)} on {device}")
    return t


def lds_limit(d: int) -> int:
    """Largest k at which a GPU step at this d combines its sums in LDS; a
    larger k adds straight to the global accumulators."""
    from . import _hip as H
    r = int(H.lib().mr_kmeans_lds_limit(int(d)))
    if r < 0:
        raise RuntimeError(f"mr_kmeans_lds_limit({d}) failed: {r}")
    return r


def _launch(X, C, n, d, k, sums, counts, cost, labels) -> None:
    from . import _hip as H
    with torch.cuda.device(X.device):
        H.call("mr_kmeans_step", H.ptr(X), H.ptr(C), n, d, k, H.ptr(sums), H.ptr(counts), H.ptr(cost),
               H.ptr(labels), H.stream(X.device))


def _spec_labels(X, C):
    X64, C64 = X.double(), C.double()
    lab = torch.empty(X.shape[0], dtype=torch.int64)
    best = torch.empty(X.shape[0], dtype=torch.float64)
    rows = max(1, (1 << 24) // C.numel())  # bounds the [rows, k, d] float64 temporary
    for i in range(0, X.shape[0], rows):  # float64 squared distances, first minimum
        D = ((X64[i:i + rows, None, :] - C64[None]) ** 2).sum(-1)
        j = D.argmin(dim=1)
        lab[i:i + rows] = j
        best[i:i + rows] = D.gather(1, j[:, None])[:, 0]
    return lab, best


def step(X: torch.Tensor, C: torch.Tensor, sums=None, counts=None, cost=None, labels: bool = False):
    """One assign-and-accumulate step; returns ``(sums, counts, cost, labels | None)``.
    Accumulators that are given are added into."""
    n, d, k = _check(X, C)
    dev = X.device
    sums = _acc(sums, (k, d), torch.float64, dev, "sums")
    counts = _acc(counts, (k,), torch.int64, dev, "counts")
    cost = _acc(cost, (1,), torch.float64, dev, "cost")
    if X.is_cuda:
        lab = torch.empty(n, dtype=torch.int32, device=dev) if labels else None
        _launch(X, C, n, d, k, sums, counts, cost, lab)
        return sums, counts, cost, lab
    lab, best = _spec_labels(X, C)
    sums.index_add_(0, lab, X.double())
    counts.index_add_(0, lab, torch.ones(n, dtype=torch.int64))
    cost += best.sum()
    return sums, counts, cost, (lab.to(torch.int32) if labels else None)


def assign(X: torch.Tensor, C: torch.Tensor) -> torch.Tensor:
    """int32 label of every row of X: its nearest centroid (lowest index on ties)."""
    n, d, k = _check(X, C)
    if X.is_cuda:
        lab = torch.empty(n, dtype=torch.int32, device=X.device)
        _launch(X, C, n, d, k, None, None, None, lab)
        return lab
    return _spec_labels(X, C)[0].to(torch.int32)
