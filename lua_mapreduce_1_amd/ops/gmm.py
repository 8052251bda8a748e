"""One EM step of a diagonal-covariance Gaussian mixture (csrc/hip/gmm.hip):
per-point log-density, arg-max component and the sufficient statistics of the
M-step, with both matrix products on the fp32 matrix cores and the n x k
responsibilities never leaving registers.

Parameters are ``weights`` [k], ``means`` [k, d], ``variances`` [k, d]: fp32,
weights > 0, variances > 0.  ``prepare`` turns them into ``A`` [k, 2d] and ``b``
[k] (fp32) with

    s_j(x) = b_j + sum_c A[j, c] x_c + sum_c A[j, d + c] x_c^2
    A[j, c] = mu_jc / var_jc,   A[j, d + c] = -1/2 / var_jc,
    b_j = log w_j - 1/2 sum_c (log(2 pi var_jc) + mu_jc^2 / var_jc),

``A`` the float64 quotient rounded once to fp32 (the same bits on the device
and on the CPU), ``b`` evaluated in float64 and rounded once (the device's
``log`` may differ from the host's in the last float64 place, so ``b`` may
differ by one fp32 ulp between the two).  **Everything below is defined against
the A, b that prepare returns**, as the bf16 k-means path is against ``C_T``.

``estep(X, weights, means, variances)`` returns ``(nk, s1, s2, ll, logp,
labels | None)``: ``logp_i = log sum_j exp s_j(x_i)`` (fp32 [n]), ``labels_i``
the arg-max component (int32), and, with ``r_ij = exp(s_ij - logp_i)``, the
float64 sums ``nk[j] = sum_i r_ij``, ``s1[j, c] = sum_i r_ij x_ic``, ``s2[j, c]
= sum_i r_ij x_ic^2``, ``ll = sum_i logp_i``; accumulators that are given are
added into.  ``score_samples`` and ``predict`` run the first pass only.

Supported: contiguous fp32 ``X`` [n, d] and parameters on one device, 1 <= d
<= 128, 1 <= k <= 4096, n >= 0.  Anything else raises; on a GPU there is no
torch fallback.  Out of scope: bf16 points, d > 128, full or tied covariances,
and several GPUs beyond what the tensor plane gives examples/GaussianMixture.
CPU tensors run the executable specification below (float64 scores from the
fp32 A, b, ``torch.logsumexp``, float64 sums).  Positivity of the weights and
variances is checked by value (on a GPU one small read, skipped while a graph
is being captured; the launches themselves neither synchronise nor allocate).

Numeric contract (u = 2^-24, gamma_m = m u / (1 - m u), gamma'_m the same with
u' = 2^-53; every "64" quantity is the float64 evaluation with the returned
fp32 A, b):

* ``e_ij = gamma_{2d+2} (|b_j| + sum_c |A[j,c] x_c| + sum_c |A[j,d+c]| x_c^2)``,
  ``e_i = max_j e_ij``: the exact fp32 fma chain of length 2d on the matrix
  unit, the one rounding of x^2 and the add of b.
* logp: ``|logp_i - logp64_i| <= B_i = 2 e_i + (k + 8) u + 4 u |logp64_i|``:
  the score error (once through the max, once through the terms), a positive
  sum of k terms, and ``expf`` / ``logf``, which HIP's math API table gives as
  1 ulp = 2 u each.  Derivation for this kernel: a lane's running sum takes at
  most k/16 terms and k/64 rescalings, the 16 lanes of a row are merged in 4
  steps of (one non-trivial ``expf``, one multiply, one add; the other factor
  is ``expf(0) = 1``), each on the smaller half of the sum, then one ``logf``
  and one add: at most (k/16 + 3 k/64 + 12) u relative on the sum plus
  ``2 u |log l| + u |logp|`` — inside ``(k + 8) u + 4 u |logp|`` for k >= 5, and
  at k < 5 the lanes hold one term each, ``l`` is 1 exactly before the merges
  and at most 4 (5 u) + 1 roundings occur.  The bound is derived, not fitted.
* labels: ``labels_i`` IS the float64 arg-max wherever the float64 margin
  between the two best scores exceeds ``2 e_i``.  Equal fp32 scores (identical
  components always tie) go to the lowest index.
* statistics: with ``rho_i = expm1(2 B_i) + 4 u`` (score and logp error through
  ``exp``, the two subtractions' roundings and ``expf``),
  ``|s1[j,c] - s1_64[j,c]| <= sum_i (rho_i + gamma_RUN + gamma'_n) r64_ij |x_ic|
  + n 2^-126 max|x|`` — the last term is the underflow floor of r — and
  likewise ``s2`` with x^2 and ``nk`` with 1.  ``RUN`` (4096) is the most terms
  an fp32 accumulator sums before it is widened to float64.
* ll: within ``sum_i B_i + gamma'_n sum_i |logp_i|`` of ``sum_i logp64_i``.
* non-finite inputs: unspecified (labels stay inside [0, k)).

``e_i`` grows with ``sum_c x_c^2 / var_c``: the quadratic is expanded, so the
terms of a score cancel and its error is relative to their size, not to the
score.  Centre (or standardise) the data first; there is no centring path here.
"""
from __future__ import annotations

import math

import numpy as np
import torch

MAX_D = 128
MAX_K = 4096
RUN = 4096


def _check(X, weights, means, variances) -> tuple[int, int, int]:
    for name, t, dim in (("X", X, 2), ("weights", weights, 1), ("means", means, 2), ("variances", variances, 2)):
        if t is None and name == "X":
            continue
        if not isinstance(t, torch.Tensor):
            raise TypeError(f"gmm: {name} must be a torch tensor (got {type(t).__name__})")
        if t.dtype != torch.float32:
            raise TypeError(f"gmm: {name} must be float32 (got {t.dtype})")
        if t.dim() != dim:
            raise ValueError(f"gmm: {name} must be {dim}-D (got {tuple(t.shape)})")
        if not t.is_contiguous():
            raise ValueError(f"gmm: {name} must be contiguous")
        if t.device != means.device:
            raise ValueError(f"gmm: {name} is on {t.device}, means on {means.device}")
    k, d = means.shape
    if not 1 <= d <= MAX_D:
        raise ValueError(f"gmm: d = {d} is outside 1..{MAX_D}")
    if not 1 <= k <= MAX_K:
        raise ValueError(f"gmm: k = {k} is outside 1..{MAX_K}")
    if tuple(variances.shape) != (k, d) or tuple(weights.shape) != (k,):
        raise ValueError(f"gmm: means {(k, d)} need variances {(k, d)} and weights {(k,)} "
                         f"(got {tuple(variances.shape)}, {tuple(weights.shape)})")
    if X is not None and X.shape[1] != d:
        raise ValueError(f"gmm: X has d = {X.shape[1]}, means have d = {d}")
    if not (means.is_cuda and torch.cuda.is_current_stream_capturing()):
        for name, t in (("weights", weights), ("variances", variances)):
            if not bool((t > 0).all()):
                raise ValueError(f"gmm: {name} must be > 0 (smallest: {float(t.min())!r})")
    return (0 if X is None else X.shape[0]), d, k


def _acc(t, shape, dtype, device, name):
    if t is None:
        return torch.zeros(shape, dtype=dtype, device=device)
    if not isinstance(t, torch.Tensor) or t.dtype != dtype or tuple(t.shape) != tuple(shape) or t.device != device \
            or not t.is_contiguous():
        raise ValueError(f"gmm: {name} must be a contiguous {dtype} tensor of shape {tuple(shape)} on {device}")
    return t


def _prepare(weights, means, variances, d, k):
    dev = means.device
    if means.is_cuda:
        from . import _hip as H
        if int(H.lib().mr_gmm_run()) != RUN:
            raise RuntimeError(f"mr_gmm_run() = {H.lib().mr_gmm_run()}, ops.gmm.RUN = {RUN}")
        A = torch.empty((k, 2 * d), dtype=torch.float32, device=dev)  # torch allocations: capture-safe
        b = torch.empty(k, dtype=torch.float32, device=dev)
        with torch.cuda.device(dev):
            H.call("mr_gmm_prepare", H.ptr(weights), H.ptr(means), H.ptr(variances), d, k, H.ptr(A), H.ptr(b),
                   H.stream(dev))
        return A, b
    M, V = means.double(), variances.double()
    A = torch.cat([M / V, -0.5 / V], dim=1).float()
    b = (weights.double().log() - 0.5 * ((2 * math.pi * V).log() + M * M / V).sum(1)).float()
    return A, b


def prepare(weights: torch.Tensor, means: torch.Tensor, variances: torch.Tensor):
    """``(A fp32 [k, 2d], b fp32 [k])`` of the score GEMM (module docstring).  On
    a GPU this is the prologue launch of every step; on CPU tensors it is the
    specification of that launch (``A`` bit for bit)."""
    _n, d, k = _check(None, weights, means, variances)
    return _prepare(weights, means, variances, d, k)


def _score(X, A, b, n, d, k, ll, labels):
    """Pass 1 on the device: (logp, labels | None); ll is added into when given."""
    from . import _hip as H
    logp = torch.empty(n, dtype=torch.float32, device=X.device)
    lab = torch.empty(n, dtype=torch.int32, device=X.device) if labels else None
    with torch.cuda.device(X.device):
        H.call("mr_gmm_score", H.ptr(X), H.ptr(A), H.ptr(b), n, d, k, H.ptr(logp), H.ptr(lab), H.ptr(ll),
               H.stream(X.device))
    return logp, lab


def _spec(X, A, b, stats: bool):
    """The executable specification: float64 scores from the fp32 A, b, in row
    blocks that bound the [rows, k] temporaries.  x^2 is the fp32 square."""
    n, d = X.shape
    k = A.shape[0]
    A64, b64 = A.double(), b.double()
    logp = torch.empty(n, dtype=torch.float64)
    lab = torch.empty(n, dtype=torch.int64)
    nk, s1, s2 = (torch.zeros(s, dtype=torch.float64) for s in ((k,), (k, d), (k, d)))
    rows = max(1, (1 << 22) // k)
    for i in range(0, n, rows):
        x, x2 = X[i:i + rows].double(), (X[i:i + rows] * X[i:i + rows]).double()
        S = torch.cat([x, x2], dim=1) @ A64.T + b64
        lp = torch.logsumexp(S, dim=1)
        logp[i:i + rows] = lp
        lab[i:i + rows] = torch.from_numpy(np.argmax(S.numpy(), axis=1))  # first maximum: the lowest index
        if stats:
            R = (S - lp[:, None]).exp()
            nk += R.sum(0)
            s1 += R.T @ x
            s2 += R.T @ x2
    return logp, lab, nk, s1, s2


def estep(X: torch.Tensor, weights: torch.Tensor, means: torch.Tensor, variances: torch.Tensor, nk=None, s1=None,
          s2=None, ll=None, labels: bool = False):
    """One E-step; returns ``(nk, s1, s2, ll, logp, labels | None)``.
    Accumulators that are given are added into (and returned by identity)."""
    n, d, k = _check(X, weights, means, variances)
    dev = X.device
    nk = _acc(nk, (k,), torch.float64, dev, "nk")
    s1 = _acc(s1, (k, d), torch.float64, dev, "s1")
    s2 = _acc(s2, (k, d), torch.float64, dev, "s2")
    ll = _acc(ll, (1,), torch.float64, dev, "ll")
    A, b = _prepare(weights, means, variances, d, k)
    if X.is_cuda:
        from . import _hip as H
        logp, lab = _score(X, A, b, n, d, k, ll, labels)
        with torch.cuda.device(dev):
            H.call("mr_gmm_stats", H.ptr(X), H.ptr(A), H.ptr(b), H.ptr(logp), n, d, k, H.ptr(nk), H.ptr(s1),
                   H.ptr(s2), H.stream(dev))
        return nk, s1, s2, ll, logp, lab
    logp, lab, dnk, ds1, ds2 = _spec(X, A, b, True)
    nk += dnk
    s1 += ds1
    s2 += ds2
    ll += logp.sum()
    return nk, s1, s2, ll, logp.float(), (lab.to(torch.int32) if labels else None)


def _first_pass(X, weights, means, variances, labels):
    n, d, k = _check(X, weights, means, variances)
    A, b = _prepare(weights, means, variances, d, k)
    if X.is_cuda:
        return _score(X, A, b, n, d, k, None, labels)
    logp, lab = _spec(X, A, b, False)[:2]
    return logp.float(), lab.to(torch.int32)


def score_samples(X: torch.Tensor, weights: torch.Tensor, means: torch.Tensor, variances: torch.Tensor):
    """fp32 log-density of every row of X under the mixture."""
    return _first_pass(X, weights, means, variances, False)[0]


def predict(X: torch.Tensor, weights: torch.Tensor, means: torch.Tensor, variances: torch.Tensor):
    """int32 arg-max component of every row of X (lowest index on ties)."""
    return _first_pass(X, weights, means, variances, True)[1]
