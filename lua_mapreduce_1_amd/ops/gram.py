"""Second-moment statistics of a tall matrix (csrc/hip/gram.hip): the column
sums and the Gram matrix of ``Z = [X | Y]`` in float64, with the products on
the fp32 matrix cores, and the small float64 algebra that turns them into a
covariance, principal components or ridge coefficients.

``moments(X, Y=None, shift=None, s=None, G=None, slabs=None)`` returns ``(s,
G)``: with ``zc = fl32(z - shift)`` (ONE fp32 subtraction per element; without a
shift ``zc = z``),

    s[c]    += sum_r zc[r, c]                 float64 [w],     w = d + t
    G[i, j] += sum_r zc[r, i] zc[r, j]        float64 [w, w],  both triangles

Accumulators that are given are added into and returned by identity, so a data
set is folded in piece by piece.  Supported: contiguous fp32 ``X`` [n, d],
``Y`` [n, t], ``shift`` [w] on one device, 1 <= d, 0 <= t, w <= ``MAX_W`` = 256,
0 <= n < 2^40.  Anything else raises; on a GPU there is no torch fallback.  CPU
tensors run the executable specification: ``Zc = Z - shift`` in fp32, then
``Zc.double()`` sums and ``Zc^T Zc`` in float64, in row blocks.

On a GPU the rows are cut into ``slabs`` contiguous slabs of ``ceil(n / slabs)``
rows, one workgroup each, every workgroup owns a float64 partial in a workspace
this module allocates, and a second launch adds the partials in slab order (no
atomics).  ``default_slabs`` gives about two workgroups per compute unit, no
slab below four runs, and keeps the workspace under 64 MiB.

Numeric contract (u = 2^-24, gamma_m = m u / (1 - m u), gamma'_m the same with
u' = 2^-53).  Everything is defined against ``zc``, which the CPU specification
reproduces bit for bit; "64" quantities are exact sums of float64 products of
``zc``.

* ``|G[i,j] - G64[i,j]| <= (gamma_RUN + gamma'_m) sum_r |zc_ri zc_rj|`` and
  ``|s[c] - s64[c]| <= (gamma_RUN + gamma'_m) sum_r |zc_rc|``, with ``RUN`` = 4096
  and ``m = f64_adds(n, slabs) = ceil(L / 2048) + slabs``, ``L = ceil(n / slabs)``.
  Derivation from the kernels as built.  The matrix unit forms a cell as an
  fp32 fma chain over the rows (products are not rounded on their own), so a
  term passes one rounding per row added after it.  For w <= 128 a wave sums at
  most 1024 rows of a run of 4096 and the four waves' values are folded with
  three fp32 additions: at most 1027 roundings, and one fp32 value has summed
  ``RUN`` rows.  For w > 128 a wave sums 2048 rows: 2048 roundings.  Either way
  ``(1 + u)^2048 (1 + u')^m - 1 <= gamma_2048 + gamma'_m + gamma_2048 gamma'_m <=
  gamma_RUN + gamma'_m``.  Widening is exact; a cell then sees one float64
  addition per run of its slab (at most ``ceil(L / 2048)``), ``slabs`` additions
  in the reduction and one into the running state, which ``m`` covers because
  the first run and the first slab are stored, not added.  Column sums: a lane
  adds one row in four of its wave's share (at most 512 terms), then two
  shuffles and, for w <= 128, the three-wave fold: fewer roundings than a
  cell.  The constants are derived, not fitted.
* ``G`` is exactly symmetric (each value is computed once and written to both
  triangles; a running state that is symmetric stays so) and its diagonal is
  >= 0.
* Inputs whose shifted values are small integers (``|zc| <= 15``, say, so that
  a run's sums stay below 2^24) make every fp32 operation exact: the result
  EQUALS the float64 reference.
* Bitwise identical for equal inputs and equal ``slabs``.
* Non-finite inputs: unspecified.

Why ``shift``.  ``covariance`` forms ``G - s s^T / n``; with data whose mean is
large against its spread the two terms agree in their leading digits and the
fp32 products have already lost them.  Subtracting a rough centre first
removes the cancellation, and ``covariance`` is shift-invariant, so any rough
mean will do: the mean of the first few thousand rows, rounded to fp32, is
enough (examples/PCA does exactly that).
"""
from __future__ import annotations

import torch

MAX_W = 256
RUN = 4096
MAX_SLABS = 4096
_WS_CAP = 64 << 20
_SPEC_ROWS = 1 << 16


def _blocks(w: int) -> int:
    """16-column blocks the kernel for width w works on (csrc/hip/gram.hip gr_blocks)."""
    nb = -(-w // 16)
    return nb if nb <= 8 else (nb + 1) & ~1


def workspace_bytes(w: int, slabs: int) -> int:
    nb = _blocks(w)
    return 8 * (nb * (nb + 1) // 2 * 256 + 16 * nb) * slabs


def f64_adds(n: int, slabs: int) -> int:
    """``m`` of the contract: float64 additions a cell of one GPU call sees at most."""
    rows = -(-n // max(1, slabs))
    return -(-rows // (RUN // 2)) + slabs


def error_factor(n: int, slabs: int) -> float:
    """``gamma_RUN + gamma'_m`` of the contract."""
    u, u64, m = 2.0 ** -24, 2.0 ** -53, f64_adds(n, slabs)
    return RUN * u / (1 - RUN * u) + m * u64 / (1 - m * u64)


def _check(X, Y, shift) -> tuple[int, int, int]:
    for name, t, dim in (("X", X, 2), ("Y", Y, 2), ("shift", shift, 1)):
        if t is None and name != "X":
            continue
        if not isinstance(t, torch.Tensor):
            raise TypeError(f"gram: {name} must be a torch tensor (got {type(t).__name__})")
        if t.dtype != torch.float32:
            raise TypeError(f"gram: {name} must be float32 (got {t.dtype})")
        if t.dim() != dim:
            raise ValueError(f"gram: {name} must be {dim}-D (got {tuple(t.shape)})")
        if not t.is_contiguous():
            raise ValueError(f"gram: {name} must be contiguous")
        if t.device != X.device:
            raise ValueError(f"gram: {name} is on {t.device}, X on {X.device}")
    n, d = X.shape
    t = 0 if Y is None else Y.shape[1]
    if Y is not None and Y.shape[0] != n:
        raise ValueError(f"gram: X has {n} rows, Y has {Y.shape[0]}")
    if d < 1 or d + t > MAX_W:
        raise ValueError(f"gram: d = {d}, t = {t}: need 1 <= d and d + t <= {MAX_W}")
    if n >= 2 ** 40:
        raise ValueError(f"gram: n = {n} rows in one call; fold X in pieces below 2^40 rows")
    if shift is not None and shift.shape[0] != d + t:
        raise ValueError(f"gram: shift has {shift.shape[0]} entries, [X | Y] has {d + t} columns")
    return n, d, t


def _acc(t, shape, device, name):
    if t is None:
        return torch.zeros(shape, dtype=torch.float64, device=device)
    if not isinstance(t, torch.Tensor) or t.dtype != torch.float64 or tuple(t.shape) != tuple(shape) \
            or t.device != device or not t.is_contiguous():
        raise ValueError(f"gram: {name} must be a contiguous float64 tensor of shape {tuple(shape)} on {device}")
    return t


def _spec(X, Y, shift, s, G):
    """The executable specification, in row blocks that bound the float64 temporaries."""
    for i in range(0, X.shape[0], _SPEC_ROWS):
        Z = X[i:i + _SPEC_ROWS] if Y is None else torch.cat([X[i:i + _SPEC_ROWS], Y[i:i + _SPEC_ROWS]], dim=1)
        Zc = (Z if shift is None else Z - shift).double()  # the subtraction is fp32
        s += Zc.sum(0)
        P = Zc.T @ Zc  # a BLAS product need not be symmetric in its last bits: keep the upper triangle, mirrored
        G += torch.triu(P) + torch.triu(P, 1).T
    return s, G


def default_slabs(n: int, w: int, device) -> int:
    """Slabs a GPU call uses: two workgroups a compute unit, no slab below four
    runs, the workspace at most 64 MiB."""
    cus = torch.cuda.get_device_properties(device).multi_processor_count
    return max(1, min(2 * cus, n // (4 * RUN), _WS_CAP // workspace_bytes(w, 1), MAX_SLABS))


def moments(X: torch.Tensor, Y=None, shift=None, s=None, G=None, slabs=None):
    """Fold the rows of ``[X | Y] - shift`` into the running float64 column sums
    ``s`` [w] and Gram matrix ``G`` [w, w] (``None``: fresh zeros); returns ``(s, G)``."""
    n, d, t = _check(X, Y, shift)
    w, dev = d + t, X.device
    s = _acc(s, (w,), dev, "s")
    G = _acc(G, (w, w), dev, "G")
    if slabs is not None and (isinstance(slabs, bool) or not isinstance(slabs, int) or not 1 <= slabs <= MAX_SLABS):
        raise ValueError(f"gram: slabs = {slabs!r} is outside 1..{MAX_SLABS}")
    if not X.is_cuda:
        return _spec(X, Y, shift, s, G)
    if n == 0:
        return s, G
    from . import _hip as H
    with torch.cuda.device(dev):
        if int(H.lib().mr_gram_run()) != RUN:
            raise RuntimeError(f"mr_gram_run() = {H.lib().mr_gram_run()}, ops.gram.RUN = {RUN}")
        S = default_slabs(n, w, dev) if slabs is None else slabs
        nbytes = int(H.lib().mr_gram_workspace_bytes(w, S))
        if nbytes != workspace_bytes(w, S):
            raise RuntimeError(f"mr_gram_workspace_bytes({w}, {S}) = {nbytes}")
        ws = torch.empty(nbytes, dtype=torch.uint8, device=dev)  # a torch allocation: capture-safe
        H.call("mr_gram_moments", H.ptr(X), H.ptr(Y) if t else None, H.ptr(shift), n, d, t, S, H.ptr(ws), H.ptr(s),
               H.ptr(G), H.stream(dev))
    return s, G


# ---- float64 algebra on the statistics (plain torch on either device: the matrices are tiny) ----

def covariance(n: int, s: torch.Tensor, G: torch.Tensor, ddof: int = 1) -> torch.Tensor:
    """``(G - s s^T / n) / (n - ddof)``: the covariance of the rows, whatever shift they were folded with."""
    if n - ddof <= 0:
        raise ValueError(f"gram: covariance of n = {n} rows with ddof = {ddof}")
    return (G - torch.outer(s, s) / n) / (n - ddof)


def pca(n: int, s: torch.Tensor, G: torch.Tensor, k: int):
    """``(components [k, w], explained_variance [k], mean_offset [w])``: the k leading eigenvectors
    of the covariance, largest eigenvalue first, each with its largest-magnitude entry positive;
    ``mean_offset = s / n`` is the mean of the shifted data (add the shift for the mean of the data)."""
    w = s.shape[0]
    if not 1 <= k <= w:
        raise ValueError(f"gram: k = {k} components of {w} columns")
    val, vec = torch.linalg.eigh(covariance(n, s, G))
    comp = vec.flip(1).T[:k].contiguous()
    big = comp.gather(1, comp.abs().argmax(dim=1, keepdim=True))
    comp = comp * torch.where(big < 0, -1.0, 1.0)
    return comp, val.flip(0)[:k].contiguous(), s / n


def ridge(n: int, s: torch.Tensor, G: torch.Tensor, d: int, lam: float = 0.0, shift=None):
    """``(coef [d, t], intercept [t])`` of ``Y ~ X coef + intercept`` from the centred normal equations
    ``(Sxx + lam I) coef = Sxy`` by Cholesky (``lam`` = 0: least squares; the intercept is not penalised).
    ``shift`` is the one the statistics were folded with, so that the intercept refers to the data."""
    w = s.shape[0]
    if not 1 <= d < w:
        raise ValueError(f"gram: d = {d} features of {w} columns leaves no target")
    C = G - torch.outer(s, s) / n
    A = C[:d, :d] + lam * torch.eye(d, dtype=torch.float64, device=G.device)
    coef = torch.cholesky_solve(C[:d, d:], torch.linalg.cholesky(A))
    mean = s / n if shift is None else s / n + shift.double()
    return coef, mean[d:] - mean[:d] @ coef
