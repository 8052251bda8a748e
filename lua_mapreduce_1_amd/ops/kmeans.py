"""The map step of Lloyd's k-means: nearest-centroid assignment and the
per-cluster partial sums in ONE launch (csrc/hip/kmeans.hip: distances on the
fp32 matrix cores, argmin in registers, sums combined in LDS; the n x k
distance matrix never exists).  bf16 points run on the 16-bit matrix cores
against fp32 centroids split into ``terms`` bf16 pieces
(csrc/hip/kmeans_bf16.hip: a small prologue launch splits, then the same plan).

``step(X, C)`` assigns every row of ``X`` [n, d] to its nearest row of ``C``
[k, d] and adds, into float64 ``sums`` [k, d], int64 ``counts`` [k] and float64
``cost`` [1], the members' coordinate sums, their number and the sum of squared
distances.  ``assign(X, C)`` is the labels-only mode of the same kernel.

Supported: contiguous fp32 or bf16 ``X`` and fp32 ``C`` on one device,
1 <= d <= 512, 1 <= k <= 4096, n >= 0; ``terms`` in {1, 2, 3} with a bf16
``X``, 3 with an fp32 ``X`` (which runs exactly as it always has).  Anything
else raises; on a GPU there is no torch fallback.  CPU tensors run the executable specification below (float64
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

bf16 ``X`` (u~ = 2^-23, gamma~_m = m u~ / (1 - m u~)).  ``split_centroids``
writes c = c(1) + c(2) + c(3) + rest, piece t the bf16 round-to-nearest-even of
the residual the pieces before it leave (the residual is exact in fp32), and
the path minimises the fp32 score against **C_T** = the sum of the first
``terms`` pieces, which is exactly representable in fp32:

* labels: the chosen centroid is within
  ``E_i(T) = 2 gamma~_{T d + 2} (|x_i| + max_j |C_T[j]|)^2`` of the float64
  minimum squared distance to C_T, and IS the float64 argmin over C_T wherever
  the float64 margin exceeds ``E_i(T)``.  Ties go to the lowest index.
* the model behind u~: every bf16 x bf16 product is exact in fp32, and the
  matrix unit's accumulation of m exact terms, in any internal order and with
  truncation allowed, errs by at most gamma~_m sum |terms|; ``|C_T[j]|^2`` is
  one length-d fp32 fma chain and the score one more fma.  This is a model of
  the hardware: it is derived, not measured.
* T = 3: C_T = C exactly whenever no piece is a bf16 subnormal; centroid
  coordinates with 0 < |c| < 2^-100 are unspecified.  T = 2 and T = 1 keep 16
  and 8 significant bits of every centroid coordinate: the answer is the
  clustering against C_T, which ``split_centroids`` returns.
* counts, sums and cost keep the bounds above with ``E_i(T)`` for ``E_i``
  (cost against the float64 cost over C_T).

Seeding (k-means||, Bahmani et al., "Scalable K-Means++";
csrc/hip/kmeans_seed.hip).  ``min_dist(X, C, mind, near, base)`` folds the new
candidates ``C`` [m, d], 1 <= m <= 16384, into every point's running nearest-
candidate squared distance ``mind`` (fp32) and index ``near`` (int32, ``base +
j``; an earlier candidate keeps a tie) and returns ``phi``, the float64 sum of
``mind`` after the fold.  ``sample`` draws the next batch from it, ``recluster``
reduces the weighted candidates to k seeds on the host, ``seed`` drives the
rounds on one device.  bf16 points are widened exactly to fp32 and run the fp32
matrix path; a bf16-MFMA seeding path is out of scope.  With ``E_i`` as above
(``max_j`` over this call's ``C``), ``D_i`` the float64 minimum squared
distance to ``C`` and ``B_i = E_i + gamma_{d+2} |x_i|^2 + 2 u (D_i + E_i)``
(the score, ``fl(|x|^2)``, and the final add and clamp):

* after one call from fresh state ``|mind_i - D_i| <= B_i``;
* over several calls ``D64[i, near_i]`` is within ``2 B_i`` of the float64
  minimum over all candidates seen (``B_i`` with ``max_j`` over all of them),
  and ``near_i`` IS that argmin wherever the float64 margin exceeds ``2 B_i``;
* ``phi`` equals the float64 sum of the returned ``mind`` to within
  ``gamma'_n sum mind`` (u' = 2^-53), and is bitwise reproducible for equal
  inputs on one device (fixed slots, fixed order, no float atomics);
* ``sample`` is exact.  Point ``i``, global index ``g = offset + i``, is
  selected iff ``phi != 0`` and ``float64(u24) * phi < (ell 2^24) *
  float64(mind_i)``, one IEEE multiply a side, where ``u24`` is the top 24 bits
  of ``F(F(F(F(seed + 0x9E3779B9) ^ round) ^ hi32(g)) ^ lo32(g))`` in 32-bit
  arithmetic and ``F`` is murmur3's finaliser (``h ^= h >> 16; h *= 0x85EBCA6B;
  h ^= h >> 13; h *= 0xC2B2AE35; h ^= h >> 16``).  ``F`` is a bijection, so
  over 2^32 consecutive ``g`` every ``u24`` occurs equally often.  Given the
  same ``mind``, ``phi`` and integers, the GPU and the CPU path (``_u24``
  below: the specification, bit for bit) return identical ``idx`` (ascending
  global indices) and ``rows`` (fp32, ``X[idx - offset]`` widened).
"""
from __future__ import annotations

import numpy as np
import torch

MAX_D = 512
MAX_K = 4096
MAX_M = 16384


def _check(X: torch.Tensor, C: torch.Tensor, terms: int = 3, limit: int = MAX_K,
           rows: str = "k") -> tuple[int, int, int]:
    for name, t in (("X", X), ("C", C)):
        if not isinstance(t, torch.Tensor):
            raise TypeError(f"kmeans: {name} must be a torch tensor (got {type(t).__name__})")
        if t.dtype != torch.float32 and (name == "C" or t.dtype != torch.bfloat16):
            raise TypeError(f"kmeans: {name} must be float32{' or bfloat16' if name == 'X' else ''} (got {t.dtype})")
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
    if not 1 <= k <= limit:
        raise ValueError(f"kmeans: {rows} = {k} is outside 1..{limit}")
    if terms not in (1, 2, 3):
        raise ValueError(f"kmeans: terms = {terms!r} is not 1, 2 or 3")
    if X.dtype == torch.float32 and terms != 3:
        raise ValueError("kmeans: terms applies to bfloat16 points; float32 points take terms = 3")
    return n, d, k


def _acc(t, shape, dtype, device, name):
    if t is None:
        return torch.zeros(shape, dtype=dtype, device=device)
    if t.dtype != dtype or tuple(t.shape) != tuple(shape) or t.device != device or not t.is_contiguous():
        raise ValueError(f"kmeans: {name} must be a contiguous {dtype} tensor of shape {tuple(shape)} on {device}")
    return t


def lds_limit(d: int, dtype: torch.dtype = torch.float32) -> int:
    """Largest k at which a GPU step at this d, on points of this dtype,
    combines its sums in LDS; a larger k adds straight to the global
    accumulators."""
    from . import _hip as H
    if dtype not in (torch.float32, torch.bfloat16):
        raise TypeError(f"kmeans: points are float32 or bfloat16 (got {dtype})")
    name = "mr_kmeans_lds_limit" if dtype == torch.float32 else "mr_kmeans_bf16_lds_limit"
    r = int(getattr(H.lib(), name)(int(d)))
    if r < 0:
        raise RuntimeError(f"{name}({d}) failed: {r}")
    return r


def _workspace(C, d, k, terms):
    """The bf16 step's workspace (csrc/hip/kmeans_bf16.hip): bf16 planes
    [terms, kpad, wd], then fp32 cn [kpad].  A torch allocation, so a step is
    capture-safe under ``torch.cuda.graph``."""
    from . import _hip as H
    kpad, wd = -(-k // 64) * 64, -(-d // 32) * 32
    nbytes = int(H.lib().mr_kmeans_bf16_workspace_bytes(d, k, terms))
    if nbytes != 2 * terms * kpad * wd + 4 * kpad:
        raise RuntimeError(f"mr_kmeans_bf16_workspace_bytes({d}, {k}, {terms}) = {nbytes}")
    ws = torch.empty(nbytes, dtype=torch.uint8, device=C.device)
    planes = ws[:nbytes - 4 * kpad].view(torch.bfloat16).view(terms, kpad, wd)
    return ws, planes[:, :k, :d], ws[nbytes - 4 * kpad:].view(torch.float32)[:k]


def _launch(X, C, n, d, k, sums, counts, cost, labels, terms=3) -> None:
    from . import _hip as H
    with torch.cuda.device(C.device):
        if X is None or X.dtype == torch.bfloat16:
            ws, planes, cn = _workspace(C, d, k, terms)
            H.call("mr_kmeans_bf16_step", H.ptr(X), H.ptr(C), n, d, k, terms, H.ptr(ws), H.ptr(sums),
                   H.ptr(counts), H.ptr(cost), H.ptr(labels), H.stream(C.device))
            return planes, cn
        H.call("mr_kmeans_step", H.ptr(X), H.ptr(C), n, d, k, H.ptr(sums), H.ptr(counts), H.ptr(cost),
               H.ptr(labels), H.stream(X.device))


def _fma32(s, v):
    """fl32(s + v * v) in one rounding, on fp32 tensors whose v has at most 24
    significant bits: the product is exact in float64, the float64 sum is
    rounded to odd (TwoSum gives the sign of what it lost), and 53 >= 24 + 2
    bits make the second rounding, to fp32, the correct one."""
    s64, p = s.double(), v.double() * v.double()
    t = s64 + p
    b = t - s64
    err = (s64 - (t - b)) + (p - b)
    inf = torch.full_like(t, float("inf"))
    odd = (t.view(torch.int64) & 1).bool()
    t = torch.where((err != 0) & ~odd, torch.nextafter(t, torch.where(err > 0, inf, -inf)), t)
    return t.float()


def split_centroids(C: torch.Tensor, terms: int = 3):
    """``(pieces bf16 [terms, k, d], cn fp32 [k])``: piece t is the bf16
    round-to-nearest-even of ``C`` minus the pieces before it, and ``cn[j]`` is
    ``|C_T[j]|^2``, C_T the sum of the pieces, as one length-d fp32 fma chain
    in column order.  On a GPU this is the prologue kernel of a bf16 step; on
    CPU tensors it is the specification of that kernel, bit for bit."""
    _n, d, k = _check(C[:0].to(torch.bfloat16), C, terms)
    if C.is_cuda:
        planes, cn = _launch(None, C, 0, d, k, None, None, None, None, terms)
        return planes.contiguous(), cn.contiguous()
    pieces, rest, ct = [], C.clone(), torch.zeros_like(C)
    for _ in range(terms):
        pieces.append(rest.to(torch.bfloat16))  # round to nearest even
        rest = rest - pieces[-1].float()        # exact
        ct = ct + pieces[-1].float()            # exact
    cn = torch.zeros(k, dtype=torch.float32)
    for c in range(d):
        cn = _fma32(cn, ct[:, c])
    return torch.stack(pieces), cn


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


def _spec_centroids(X, C, terms):
    """The centroids the CPU specification measures against: C, or C_T for bf16 points."""
    return C if X.dtype == torch.float32 else split_centroids(C, terms)[0].float().sum(0)


def step(X: torch.Tensor, C: torch.Tensor, sums=None, counts=None, cost=None, labels: bool = False, terms: int = 3):
    """One assign-and-accumulate step; returns ``(sums, counts, cost, labels | None)``.
    Accumulators that are given are added into.  ``terms``: the bf16 pieces of
    every centroid a bf16 ``X`` is measured against (see the contract above)."""
    n, d, k = _check(X, C, terms)
    dev = X.device
    sums = _acc(sums, (k, d), torch.float64, dev, "sums")
    counts = _acc(counts, (k,), torch.int64, dev, "counts")
    cost = _acc(cost, (1,), torch.float64, dev, "cost")
    if X.is_cuda:
        lab = torch.empty(n, dtype=torch.int32, device=dev) if labels else None
        _launch(X, C, n, d, k, sums, counts, cost, lab, terms)
        return sums, counts, cost, lab
    lab, best = _spec_labels(X, _spec_centroids(X, C, terms))
    sums.index_add_(0, lab, X.double())
    counts.index_add_(0, lab, torch.ones(n, dtype=torch.int64))
    cost += best.sum()
    return sums, counts, cost, (lab.to(torch.int32) if labels else None)


def assign(X: torch.Tensor, C: torch.Tensor, terms: int = 3) -> torch.Tensor:
    """int32 label of every row of X: its nearest centroid (lowest index on ties)."""
    n, d, k = _check(X, C, terms)
    if X.is_cuda:
        lab = torch.empty(n, dtype=torch.int32, device=X.device)
        _launch(X, C, n, d, k, None, None, None, lab, terms)
        return lab
    return _spec_labels(X, _spec_centroids(X, C, terms))[0].to(torch.int32)


# ---- k-means|| seeding (csrc/hip/kmeans_seed.hip; contract in the module docstring) -------------

_M32 = 0xFFFFFFFF


def _fmix(h):
    """murmur3's 32-bit finaliser on a Python int or a uint64 array of 32-bit values."""
    h = h ^ (h >> 16)
    h = (h * 0x85EBCA6B) & _M32
    h = h ^ (h >> 13)
    h = (h * 0xC2B2AE35) & _M32
    return h ^ (h >> 16)


def _u24(seed: int, round: int, g: np.ndarray) -> np.ndarray:
    """The sampling hash: top 24 bits of F(F(F(F(seed + 0x9E3779B9) ^ round) ^ hi32(g)) ^ lo32(g))."""
    g = np.asarray(g, dtype=np.uint64)
    hs = np.uint64(_fmix(_fmix((int(seed) + 0x9E3779B9) & _M32) ^ (int(round) & _M32)))
    return _fmix(_fmix(hs ^ (g >> np.uint64(32))) ^ (g & np.uint64(_M32))) >> np.uint64(8)


def selected(mind, phi: float, ell: float, seed: int, round: int, g) -> np.ndarray:
    """The selection rule on host arrays: ``mind`` of the points with global indices ``g``."""
    with np.errstate(invalid="ignore"):
        lhs = _u24(seed, round, g).astype(np.float64) * np.float64(phi)
        return (np.float64(phi) != 0) & (lhs < np.float64(float(ell) * 2.0 ** 24) * np.asarray(mind, dtype=np.float64))


def _state(t, n, dtype, fill, device, name):
    return torch.full((n,), fill, dtype=dtype, device=device) if t is None else _acc(t, (n,), dtype, device, name)


def min_dist(X: torch.Tensor, C: torch.Tensor, mind=None, near=None, base: int = 0):
    """Fold the new candidates ``C`` into ``mind`` / ``near`` (``None``: fresh
    state, +inf / -1; given tensors are updated in place); returns
    ``(mind, near, phi)``, ``phi`` float64 [1]."""
    n, d, m = _check(X, C, limit=MAX_M, rows="m")
    dev = X.device
    mind = _state(mind, n, torch.float32, float("inf"), dev, "mind")
    near = _state(near, n, torch.int32, -1, dev, "near")
    if not 0 <= int(base) <= 2 ** 31 - 1 - m:
        raise ValueError(f"kmeans: base = {base!r} with m = {m} leaves int32")
    phi = torch.empty(1, dtype=torch.float64, device=dev)
    if X.is_cuda:
        from . import _hip as H
        with torch.cuda.device(dev):
            part = torch.empty(int(H.lib().mr_kmeans_seed_partials()), dtype=torch.float64, device=dev)
            H.call("mr_kmeans_min_dist", H.ptr(X), int(X.dtype == torch.bfloat16), H.ptr(C), n, d, m, H.ptr(mind),
                   H.ptr(near), int(base), H.ptr(part), H.ptr(phi), H.stream(dev))
        return mind, near, phi
    lab, best = _spec_labels(X, C)
    dist = best.float()
    take = dist < mind  # strict: an earlier candidate keeps a tie
    mind[take] = dist[take]
    near[take] = (int(base) + lab[take]).to(torch.int32)
    phi[0] = mind.double().sum()
    return mind, near, phi


def sample(X: torch.Tensor, mind: torch.Tensor, phi, ell: float, seed: int, round: int, offset: int = 0):
    """Bernoulli D^2 sampling: ``(idx int64 [s], rows fp32 [s, d])``, the
    selected points' global indices ``offset + i``, ascending, and their rows."""
    if not isinstance(X, torch.Tensor) or X.dtype not in (torch.float32, torch.bfloat16):
        raise TypeError("kmeans: X must be a float32 or bfloat16 torch tensor")
    if X.dim() != 2 or not X.is_contiguous() or not 1 <= X.shape[1] <= MAX_D:
        raise ValueError(f"kmeans: X must be contiguous [n, d] with d in 1..{MAX_D} (got {tuple(X.shape)})")
    n, d = X.shape
    if not isinstance(mind, torch.Tensor) or mind.dtype != torch.float32:
        raise TypeError("kmeans: mind must be a float32 torch tensor")
    _acc(mind, (n,), torch.float32, X.device, "mind")
    phi, ell, offset = float(phi), float(ell), int(offset)
    if not ell > 0 or ell == float("inf"):
        raise ValueError(f"kmeans: ell = {ell!r} is not a positive finite number")
    if not 0 <= offset <= 2 ** 63 - 1 - n:
        raise ValueError(f"kmeans: offset = {offset!r} leaves int64")
    seed, round = int(seed) & _M32, int(round) & _M32
    if X.is_cuda:
        from . import _hip as H
        dev = X.device
        nb = -(-n // 4096)
        counts = torch.empty(nb, dtype=torch.int32, device=dev)
        offs = torch.empty(nb, dtype=torch.int64, device=dev)
        total = torch.empty(1, dtype=torch.int64, device=dev)
        rule = (offset, phi, ell * 2.0 ** 24, seed, round)
        with torch.cuda.device(dev):
            H.call("mr_kmeans_sample_count", H.ptr(mind), n, *rule, H.ptr(counts), H.ptr(offs), H.ptr(total),
                   H.stream(dev))
            s = int(total.item())  # the one synchronisation: it sizes the outputs
            idx = torch.empty(s, dtype=torch.int64, device=dev)
            rows = torch.empty((s, d), dtype=torch.float32, device=dev)
            if s:
                H.call("mr_kmeans_sample_write", H.ptr(X), int(X.dtype == torch.bfloat16), H.ptr(mind), n, d, *rule,
                       H.ptr(offs), H.ptr(idx), H.ptr(rows), H.stream(dev))
        return idx, rows
    g = np.uint64(offset) + np.arange(n, dtype=np.uint64)
    pick = torch.from_numpy(np.flatnonzero(selected(mind.numpy(), phi, ell, seed, round, g)))
    return pick + offset, X[pick].float()


def recluster(cands, weights, k: int, seed: int) -> torch.Tensor:
    """Weighted k-means++ over the candidates, in float64 numpy on the host:
    the first pick is drawn with probability proportional to weight, every
    later one to weight x D^2 (to the picks so far), from ``default_rng(seed)``.
    Returns the k picked rows, fp32, on the candidates' device."""
    dev = cands.device if isinstance(cands, torch.Tensor) else torch.device("cpu")
    P = (cands.detach().cpu().numpy() if isinstance(cands, torch.Tensor) else np.asarray(cands)).astype(np.float64)
    w = (weights.detach().cpu().numpy() if isinstance(weights, torch.Tensor) else np.asarray(weights)) \
        .astype(np.float64)
    if P.ndim != 2 or w.shape != (len(P),) or (w < 0).any():
        raise ValueError(f"kmeans: candidates {P.shape} need one weight >= 0 each (got {w.shape})")
    if int((w > 0).sum()) < int(k) or k < 1:
        raise ValueError(f"kmeans: k = {k} seeds need as many candidates of positive weight (got {int((w > 0).sum())})")
    rng = np.random.default_rng(seed)
    picks = [int(rng.choice(len(P), p=w / w.sum()))]
    D = ((P - P[picks[0]]) ** 2).sum(1)
    for _ in range(k - 1):
        p = w * D
        if not p.sum() > 0:  # the rest coincide with picks: any unpicked candidate of positive weight
            p = w.copy()
            p[picks] = 0
        picks.append(int(rng.choice(len(P), p=p / p.sum())))
        D = np.minimum(D, ((P - P[picks[-1]]) ** 2).sum(1))
        D[picks[-1]] = 0.0
    return torch.from_numpy(P[picks].astype(np.float32)).to(dev)


def seed(X: torch.Tensor, k: int, ell: float | None = None, rounds: int = 5, seed: int = 0):
    """k-means|| on one device: ``(C0 fp32 [k, d], info)``.  The first candidate
    is row ``default_rng(seed).integers(n)``; each of ``rounds`` rounds folds the
    newest batch (``min_dist``, ``base`` = the candidates so far) and samples
    the next with ``ell`` (default 2k) expected picks; the last batch is folded,
    every candidate is weighted by the points nearest to it and ``recluster``
    picks the k seeds.  ``info``: ``candidates``, ``weights``, ``phi`` per round."""
    if not isinstance(X, torch.Tensor) or X.dim() != 2 or X.shape[0] < 1:
        raise ValueError("kmeans: seed needs a non-empty [n, d] tensor of points")
    ell = 2.0 * k if ell is None else float(ell)
    first = int(np.random.default_rng(seed).integers(X.shape[0]))
    cands, batch, mind, near, phis = [], X[first:first + 1].float().contiguous(), None, None, []

    def fold(batch, mind, near):
        phi = None
        for i in range(0, len(batch), MAX_M):  # a batch beyond the kernel's range goes in pieces
            mind, near, phi = min_dist(X, batch[i:i + MAX_M].contiguous(), mind, near,
                                       base=sum(len(c) for c in cands) + i)
        cands.append(batch)
        return mind, near, phi

    for r in range(int(rounds)):
        mind, near, phi = fold(batch, mind, near)
        phis.append(float(phi))
        _idx, batch = sample(X, mind, phi, ell, seed, r)
        if len(batch) == 0:
            break
    if len(batch):
        mind, near, _phi = fold(batch, mind, near)
    cands = torch.cat(cands)
    weights = torch.bincount(near.long(), minlength=len(cands)).cpu()
    return recluster(cands, weights, k, seed), {"candidates": cands, "weights": weights, "phi": phis}
