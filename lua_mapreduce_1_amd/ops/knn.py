"""Brute-force k-nearest neighbours under the squared Euclidean metric
(csrc/hip/knn.hip: distances on the fp32 matrix cores, the K best of every query
kept in LDS behind a threshold, partial lists merged by a second kernel; the
q x n distance matrix never exists).

``search(Q, X, k)`` returns, for every row of ``Q`` [q, d], the ``k`` rows of
``X`` [n, d] nearest to it: fp32 ``dist`` [q, k], ascending, and int64 ``idx``
[q, k] = ``base + row``.  Running lists ``dist`` / ``idx`` that are given are
merged into, in place, and returned (the contract of ``ops.kmeans.min_dist``'s
running state), so ``X`` can be searched in pieces; ``merge`` joins two running
states, e.g. those of two devices.  Slots beyond the points seen hold ``+inf``
and ``-1``.  ``classify`` is the majority vote of a kNN classifier.

Supported: contiguous fp32 ``Q`` and ``X`` on one device, 1 <= d <= 512,
1 <= k <= 64, q >= 0, 0 <= n < 2^31 per call, 0 <= base with base + n inside
int64.  Anything else raises; on a GPU there is no torch fallback.  CPU tensors
run the executable specification below: float64 distances rounded once to
fp32, then a stable sort by (dist, idx).  ``slabs`` (GPU only) overrides the
number of slabs ``X`` is cut into so that few queries still fill the device; the
result does not depend on it.

Numeric contract (u = 2^-24, gamma_m = m u / (1 - m u), D = the float64 squared
distance, ``E_i = 2 gamma_{d+2} (|q_i| + max_j |x_j|)^2`` and
``B_i = E_i + gamma_{d+2} |q_i|^2 + 2 u (D + E_i)``: the score ``|x|^2 - 2 q.x``
of two length-d fma chains and one fma, ``fl(|q|^2)``, and the final add and
clamp — the bound of ``min_dist`` with the query in the point's role):

* determinism: the fp32 ``dist`` of a (query, point) pair is a function of that
  pair alone, not of the slab count, the tile position or the other rows of the
  call, and the result is exactly the k smallest (dist, idx) pairs in
  lexicographic order.  It is therefore bitwise identical for every ``slabs``
  and when ``X`` is searched in pieces through the running state or ``merge``.
* accuracy: ``|dist[i, r] - D[i, idx[i, r]]| <= B_i``.
* separation: ``max_r D[i, idx[i, r]] <= min_{j not returned} D[i, j] + 2 B_i``.
* set equality: the index set equals the float64 top-k wherever the float64 gap
  between the k-th and (k+1)-th distance exceeds ``2 B_i``.
* indices are distinct and lie in [base, base + n), or are -1.
* non-finite coordinates: unspecified, but the indices stay in range.
* inputs whose coordinates are small integers make every fp32 operation exact:
  the result then EQUALS the float64 reference sorted by (distance, index),
  ties included.
"""
from __future__ import annotations

import torch

MAX_D = 512
MAX_K = 64
MAX_SLABS = 65535
_MIN_SLAB_ROWS = 4096  # a slab pays K passes per query before its threshold bites


def _check(Q, X, k) -> tuple[int, int, int]:
    for name, t in (("Q", Q), ("X", X)):
        if not isinstance(t, torch.Tensor):
            raise TypeError(f"knn: {name} must be a torch tensor (got {type(t).__name__})")
        if t.dtype != torch.float32:
            raise TypeError(f"knn: {name} must be float32 (got {t.dtype})")
        if t.dim() != 2:
            raise ValueError(f"knn: {name} must be 2-D [rows, d] (got {tuple(t.shape)})")
        if not t.is_contiguous():
            raise ValueError(f"knn: {name} must be contiguous")
    if Q.device != X.device:
        raise ValueError(f"knn: Q is on {Q.device}, X on {X.device}")
    q, d = Q.shape
    n = X.shape[0]
    if X.shape[1] != d:
        raise ValueError(f"knn: Q has d = {d}, X has d = {X.shape[1]}")
    if not 1 <= d <= MAX_D:
        raise ValueError(f"knn: d = {d} is outside 1..{MAX_D}")
    if isinstance(k, bool) or not isinstance(k, int) or not 1 <= k <= MAX_K:
        raise ValueError(f"knn: k = {k!r} is outside 1..{MAX_K}")
    if n >= 2 ** 31:
        raise ValueError(f"knn: n = {n} rows in one call; search X in pieces below 2^31 rows")
    return q, n, d


def _state(dist, idx, q, k, device):
    """The running lists: fresh (+inf, -1), or the caller's, checked."""
    if (dist is None) != (idx is None):
        raise ValueError("knn: dist and idx come together")
    if dist is None:
        return (torch.full((q, k), float("inf"), dtype=torch.float32, device=device),
                torch.full((q, k), -1, dtype=torch.int64, device=device))
    for name, t, dtype in (("dist", dist, torch.float32), ("idx", idx, torch.int64)):
        if not isinstance(t, torch.Tensor) or t.dtype != dtype or tuple(t.shape) != (q, k) or t.device != device \
                or not t.is_contiguous():
            raise ValueError(f"knn: {name} must be a contiguous {dtype} tensor of shape {(q, k)} on {device}")
    return dist, idx


def _sorted_topk(dist, idx, k):
    """The k lexicographically smallest (dist, idx) of every row; free slots (idx < 0) last."""
    free = idx < 0
    dist = torch.where(free, torch.full_like(dist, float("inf")), dist)
    tie = torch.where(free, torch.full_like(idx, 2 ** 63 - 1), idx)
    o1 = torch.sort(tie, dim=1, stable=True).indices
    o2 = torch.sort(dist.gather(1, o1), dim=1, stable=True).indices
    order = o1.gather(1, o2)[:, :k]
    return dist.gather(1, order).contiguous(), torch.where(free, torch.full_like(idx, -1), idx).gather(1, order) \
        .contiguous()


def _spec(Q, X, k, dist, idx, base):
    q, n, d = Q.shape[0], X.shape[0], Q.shape[1]
    X64 = X.double()
    rows = max(1, (1 << 24) // max(1, n * d))  # bounds the [rows, n, d] float64 temporary
    cand = torch.arange(base, base + n, dtype=torch.int64).expand(q, n)
    D = torch.empty((q, n), dtype=torch.float32)
    for i in range(0, q, rows):
        D[i:i + rows] = ((Q[i:i + rows, None, :].double() - X64[None]) ** 2).sum(-1).float()  # rounded once
    nd, ni = _sorted_topk(torch.cat([dist, D], 1), torch.cat([idx, cand], 1), k)
    dist.copy_(nd)
    idx.copy_(ni)
    return dist, idx


def default_slabs(q: int, n: int, device) -> int:
    """Slabs of ``X`` a GPU search uses: enough (query block, slab) workgroups for two a
    compute unit, no slab below 4096 rows."""
    cus = torch.cuda.get_device_properties(device).multi_processor_count
    blocks = max(1, -(-q // 128))
    return max(1, min(-(-2 * cus // blocks), n // _MIN_SLAB_ROWS, 256))


def search(Q: torch.Tensor, X: torch.Tensor, k: int, dist=None, idx=None, base: int = 0, slabs=None):
    """Fold the rows of ``X`` (indices ``base + row``) into the queries' running
    k-nearest lists (``None``: fresh, +inf / -1; given tensors are updated in
    place); returns ``(dist, idx)``."""
    q, n, d = _check(Q, X, k)
    dev = Q.device
    dist, idx = _state(dist, idx, q, k, dev)
    if isinstance(base, bool) or not isinstance(base, int) or not 0 <= base <= 2 ** 63 - 1 - n:
        raise ValueError(f"knn: base = {base!r} with n = {n} leaves int64")
    if slabs is not None and (isinstance(slabs, bool) or not isinstance(slabs, int) or not 1 <= slabs <= MAX_SLABS):
        raise ValueError(f"knn: slabs = {slabs!r} is outside 1..{MAX_SLABS}")
    if not Q.is_cuda:
        return _spec(Q, X, k, dist, idx, base)
    from . import _hip as H
    with torch.cuda.device(dev):
        S = default_slabs(q, n, dev) if slabs is None else slabs
        S = max(1, min(S, -(-n // 64)))
        nbytes = int(H.lib().mr_knn_workspace_bytes(q, k, S))
        if nbytes != 8 * S * q * k:
            raise RuntimeError(f"mr_knn_workspace_bytes({q}, {k}, {S}) = {nbytes}")
        ws = torch.empty(nbytes, dtype=torch.uint8, device=dev)  # a torch allocation: capture-safe
        H.call("mr_knn_search", H.ptr(Q), H.ptr(X), q, n, d, k, base, S, H.ptr(ws), H.ptr(dist), H.ptr(idx),
               H.stream(dev))
    return dist, idx


def merge(dist_a: torch.Tensor, idx_a: torch.Tensor, dist_b: torch.Tensor, idx_b: torch.Tensor):
    """The k smallest (dist, idx) pairs of two running states [q, k], as new tensors."""
    if not isinstance(dist_a, torch.Tensor) or dist_a.dim() != 2 or not 1 <= dist_a.shape[1] <= MAX_K:
        raise ValueError(f"knn: dist_a must be a [q, k] tensor with k in 1..{MAX_K}")
    q, k = dist_a.shape
    dev = dist_a.device
    _state(dist_a, idx_a, q, k, dev)
    _state(dist_b, idx_b, q, k, dev)
    if not dist_a.is_cuda:
        return _sorted_topk(torch.cat([dist_a, dist_b], 1), torch.cat([idx_a, idx_b], 1), k)
    from . import _hip as H
    dist, idx = torch.empty_like(dist_a), torch.empty_like(idx_a)
    with torch.cuda.device(dev):
        H.call("mr_knn_merge", H.ptr(dist_a), H.ptr(idx_a), H.ptr(dist_b), H.ptr(idx_b), q, k, H.ptr(dist),
               H.ptr(idx), H.stream(dev))
    return dist, idx


def classify(idx: torch.Tensor, labels: torch.Tensor, num_classes: int) -> torch.Tensor:
    """int32 [q]: the majority class among ``labels[idx]``; the lowest class wins
    a tie, ``-1`` slots do not vote (a query without neighbours gets class 0).
    Plain torch on either device."""
    if not isinstance(idx, torch.Tensor) or idx.dtype != torch.int64 or idx.dim() != 2:
        raise ValueError("knn: idx must be an int64 [q, k] tensor")
    if not isinstance(labels, torch.Tensor) or labels.dim() != 1 or labels.dtype.is_floating_point \
            or labels.device != idx.device:
        raise ValueError("knn: labels must be a 1-D integer tensor on idx's device")
    if int(num_classes) < 1:
        raise ValueError(f"knn: num_classes = {num_classes!r}")
    seen = idx >= 0
    lab = labels.to(torch.int64)[idx.clamp(min=0)]
    if bool((seen & ((lab < 0) | (lab >= num_classes))).any()):
        raise ValueError(f"knn: a label is outside 0..{int(num_classes) - 1}")
    votes = torch.zeros((idx.shape[0], int(num_classes)), dtype=torch.int64, device=idx.device)
    votes.scatter_add_(1, lab.clamp(0, int(num_classes) - 1), seen.to(torch.int64))
    return votes.argmax(dim=1).to(torch.int32)  # argmax returns the first maximum: the lowest class
