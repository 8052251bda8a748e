"""Logistic regression by Newton's method (iteratively reweighted least squares):
the per-iteration statistics in one pass over the points (csrc/hip/glm.hip), with
the weighted Gram matrix on the fp32 matrix cores, and the small float64 algebra
that turns them into a Newton step and a fit.

``newton_stats(X, y, beta, ll=None, g=None, H=None, slabs=None)`` returns ``(ll, g,
H)``: with ``z_r = [x_r, 1]`` (p = d + 1 columns, the last is the intercept),
``eta_r = z_r . beta``, ``mu_r = sigmoid(eta_r)`` and ``om_r = mu_r (1 - mu_r)``,

    ll     += sum_r y_r eta_r - softplus(eta_r)     float64 [1]
    g[c]   += sum_r (y_r - mu_r) z_rc               float64 [p]
    H[i,j] += sum_r om_r z_ri z_rj                  float64 [p, p], both triangles

``H`` is the NEGATIVE Hessian of the log-likelihood.  Accumulators that are given
are added into and returned by identity.  Supported: contiguous fp32 ``X`` [n, d],
``y`` [n] (labels, or soft labels in [0, 1]: documented, not checked) and ``beta``
[d + 1] on one device, 1 <= d <= ``MAX_D`` = 127, 0 <= n < 2^40.  Anything else
raises; on a GPU there is no torch fallback.  CPU tensors run the executable
specification: the fp32 inputs widened, everything in float64, in row blocks.

On a GPU the rows are cut into ``slabs`` contiguous slabs of ``ceil(n / slabs)``
rows, one workgroup each, every workgroup owns a float64 partial in a workspace
this module allocates, and a second launch adds the partials in slab order (no
atomics), exactly as ``ops.gram`` does.  The torch form of the same map writes
four n- or n x d-sized temporaries an iteration; this one reads ``X`` once.

Numeric contract (u = 2^-24, gamma_m = m u / (1 - m u), gamma'_m the same with u' =
2^-53; "64" quantities are float64 arithmetic on the fp32 inputs; NB = ceil(p /
16)).  ``error_terms`` evaluates the three bounds.

* eta: ``|eta_r - eta64_r| <= e_r = gamma_k sum_c |z_rc beta_c|`` with ``k = NB + 4``:
  a lane multiplies once and then runs NB - 1 fmas over its blocks, and the 16
  lanes of a row are summed by a butterfly of 4 additions.
* link: ``|mu_r - mu64_r| <= d_mu_r = e_r / 4 + 3 u`` and ``|om_r - om64_r| <= d_om_r =
  e_r / (6 sqrt 3) + 4 u``.  1/4 and 1/(6 sqrt 3) are the Lipschitz constants of
  the sigmoid and of its derivative.  With ``t = expf(-|eta|)`` (1 ulp = 2 u by
  HIP's math API table, the function gmm.hip uses), ``mu = 1 / (1 + t)`` or ``t / (1
  + t)``: the error of t moves mu by at most ``2 u t / (1 + t)^2 <= u / 2``, the sum
  and the IEEE division by 2 u mu: 2.5 u.  ``om = fl(mu fl(1 - mu))``: the error
  of mu passes with slope ``|1 - 2 mu| <= 1``, two roundings of a value <= 1/4
  add u / 2: 3.5 u.  The slack covers second-order terms and a flushed t.
* H: ``|H[i,j] - H64[i,j]| <= sum_r (d_om_r (1 + G) + G om64_r) |z_ri z_rj| + 3 n
  2^-126 Z^2``, ``G = (1 + u)(1 + gamma_RUN + gamma'_m) - 1``: the rounding of the A
  operand ``om_r z_ri``, the fp32 fma chain of the matrix unit over at most 1024
  rows of a run of ``RUN`` = 4096 and the three-wave fold (see ops/gram.py), and
  ``m = f64_adds(n, slabs) = ceil(L / RUN) + slabs`` float64 additions.  The last
  term is the underflow floor in the manner of ops/gmm.py (a flushed om, A
  operand or product), ``Z = max(1, max |x|)``.
* g: ``|g[c] - g64[c]| <= sum_r (d_res_r (1 + G) + G |y_r - mu64_r|) |z_rc| + 3 n
  2^-126 Z`` with ``d_res_r = d_mu_r + u |y_r - mu64_r|`` (the subtraction): a lane
  sums at most 256 rows of a run by fma, then two shuffles and the fold.
* ll: ``|ll - ll64| <= sum_r (b_r (1 + G) + G |t64_r|) + 3 n 2^-126`` with ``t_r = y_r
  eta_r - softplus(eta_r)`` and ``b_r = (1 + |y_r|) e_r (1 + 2 u) + u (4 + |y_r
  eta64_r| + 2 softplus64_r)``: the slope of t in eta, ``log1pf`` (1 ulp) of a
  t with 2 u relative error (2.4 u together), the addition in softplus and the
  one fma.
* ``H`` is exactly symmetric (each value is computed once and written to both
  triangles) and its diagonal is >= 0 (``om >= 0``, and the products ``fl(om z) z``
  are then >= 0).
* Bitwise identical for equal inputs and equal ``slabs``.
* At ``beta = 0`` with small-integer ``X`` (``|x| <= 15``) and ``y`` in {0, 1}, ``eta``
  is 0, ``mu`` 0.5 and ``om`` 0.25 exactly and every fp32 operation on ``g`` and
  ``H`` is exact: ``H`` EQUALS ``0.25 Z^T Z`` and ``g`` ``Z^T (y - 0.5)`` as float64
  computes them.
* Finite inputs give finite outputs for every ``|eta|`` an fp32 can hold (the
  link saturates: ``t`` underflows to 0, nothing overflows) as long as the sums
  themselves stay finite.  Non-finite inputs: unspecified.

``e_r`` grows with ``sum_c |x_rc beta_c|``, not with ``|eta_r|``: columns with a large
common offset make terms that cancel in eta.  Centre or standardise ``X`` first
(one ``ops.gram.moments`` pass gives the means and variances); that is what keeps
``e_r`` small.  The intercept absorbs the shift.

Out of scope: p > 128, bf16 points, other families and links, sample weights.
"""
from __future__ import annotations

import math

import torch

MAX_D = 127
RUN = 4096
MAX_SLABS = 4096
MAX_HALVINGS = 10
_WS_CAP = 64 << 20
_SPEC_ROWS = 1 << 16
_U = 2.0 ** -24


def _blocks(p: int) -> int:
    return -(-p // 16)


def workspace_bytes(p: int, slabs: int) -> int:
    nb = _blocks(p)
    return 8 * (nb * (nb + 1) // 2 * 256 + 16 * nb + 1) * slabs


def f64_adds(n: int, slabs: int) -> int:
    """``m`` of the contract: float64 additions a cell of one GPU call sees at most."""
    rows = -(-n // max(1, slabs))
    return -(-rows // RUN) + slabs


def _check(X, y, beta) -> tuple[int, int]:
    for name, t, dim in (("X", X, 2), ("y", y, 1), ("beta", beta, 1)):
        if not isinstance(t, torch.Tensor):
            raise TypeError(f"glm: {name} must be a torch tensor (got {type(t).__name__})")
        if t.dtype != torch.float32:
            raise TypeError(f"glm: {name} must be float32 (got {t.dtype})")
        if t.dim() != dim:
            raise ValueError(f"glm: {name} must be {dim}-D (got {tuple(t.shape)})")
        if not t.is_contiguous():
            raise ValueError(f"glm: {name} must be contiguous")
        if t.device != X.device:
            raise ValueError(f"glm: {name} is on {t.device}, X on {X.device}")
    n, d = X.shape
    if not 1 <= d <= MAX_D:
        raise ValueError(f"glm: d = {d} is outside 1..{MAX_D}")
    if n >= 2 ** 40:
        raise ValueError(f"glm: n = {n} rows in one call; fold X in pieces below 2^40 rows")
    if y.shape[0] != n:
        raise ValueError(f"glm: X has {n} rows, y has {y.shape[0]}")
    if beta.shape[0] != d + 1:
        raise ValueError(f"glm: beta has {beta.shape[0]} entries, [X | 1] has {d + 1} columns")
    return n, d


def _acc(t, shape, device, name):
    if t is None:
        return torch.zeros(shape, dtype=torch.float64, device=device)
    if not isinstance(t, torch.Tensor) or t.dtype != torch.float64 or tuple(t.shape) != tuple(shape) \
            or t.device != device or not t.is_contiguous():
        raise ValueError(f"glm: {name} must be a contiguous float64 tensor of shape {tuple(shape)} on {device}")
    return t


def _rows64(X, y, beta, i):
    """Float64 quantities of the rows i .. i + _SPEC_ROWS: ``(Z, y, eta, mu, softplus)``."""
    x = X[i:i + _SPEC_ROWS].double()
    Z = torch.cat([x, torch.ones((x.shape[0], 1), dtype=torch.float64, device=x.device)], dim=1)
    eta = Z @ beta.double()
    t = torch.exp(-eta.abs())
    mu = torch.where(eta >= 0, 1 / (1 + t), t / (1 + t))
    return Z, y[i:i + _SPEC_ROWS].double(), eta, mu, eta.clamp(min=0) + torch.log1p(t)


def _spec(X, y, beta, ll, g, H):
    """The executable specification, in row blocks that bound the float64 temporaries."""
    for i in range(0, X.shape[0], _SPEC_ROWS):
        Z, yy, eta, mu, sp = _rows64(X, y, beta, i)
        ll += (yy * eta - sp).sum()
        g += Z.T @ (yy - mu)
        P = (Z * (mu * (1 - mu))[:, None]).T @ Z  # keep the upper triangle, mirrored (see ops/gram.py)
        H += torch.triu(P) + torch.triu(P, 1).T
    return ll, g, H


def default_slabs(n: int, p: int, device) -> int:
    """Slabs a GPU call uses: two workgroups a compute unit, no slab below four
    runs, the workspace at most 64 MiB."""
    cus = torch.cuda.get_device_properties(device).multi_processor_count
    return max(1, min(2 * cus, n // (4 * RUN), _WS_CAP // workspace_bytes(p, 1), MAX_SLABS))


def newton_stats(X: torch.Tensor, y: torch.Tensor, beta: torch.Tensor, ll=None, g=None, H=None, slabs=None):
    """Fold the rows of ``X``, ``y`` into the running float64 log-likelihood ``ll`` [1], gradient ``g``
    [p] and negative Hessian ``H`` [p, p] at ``beta`` (``None``: fresh zeros); returns ``(ll, g, H)``."""
    n, d = _check(X, y, beta)
    p, dev = d + 1, X.device
    ll = _acc(ll, (1,), dev, "ll")
    g = _acc(g, (p,), dev, "g")
    H = _acc(H, (p, p), dev, "H")
    if slabs is not None and (isinstance(slabs, bool) or not isinstance(slabs, int) or not 1 <= slabs <= MAX_SLABS):
        raise ValueError(f"glm: slabs = {slabs!r} is outside 1..{MAX_SLABS}")
    if not X.is_cuda:
        return _spec(X, y, beta, ll, g, H)
    if n == 0:
        return ll, g, H
    from . import _hip as Hp
    with torch.cuda.device(dev):
        if int(Hp.lib().mr_glm_run()) != RUN:
            raise RuntimeError(f"mr_glm_run() = {Hp.lib().mr_glm_run()}, ops.glm.RUN = {RUN}")
        S = default_slabs(n, p, dev) if slabs is None else slabs
        nbytes = int(Hp.lib().mr_glm_workspace_bytes(p, S))
        if nbytes != workspace_bytes(p, S):
            raise RuntimeError(f"mr_glm_workspace_bytes({p}, {S}) = {nbytes}")
        ws = torch.empty(nbytes, dtype=torch.uint8, device=dev)  # a torch allocation: capture-safe
        Hp.call("mr_glm_newton", Hp.ptr(X), Hp.ptr(y), Hp.ptr(beta), n, d, S, Hp.ptr(ws), Hp.ptr(ll), Hp.ptr(g),
                Hp.ptr(H), Hp.stream(dev))
    return ll, g, H


def error_terms(X: torch.Tensor, y: torch.Tensor, beta: torch.Tensor, slabs: int = 1):
    """The contract's bounds ``(ll_bound [1], g_bound [p], H_bound [p, p])`` (float64, on X's device)
    for one GPU call with these inputs and ``slabs``."""
    n, d = _check(X, y, beta)
    p, dev = d + 1, X.device
    k, m = _blocks(p) + 4, f64_adds(n, slabs)
    gk = k * _U / (1 - k * _U)
    G = (1 + _U) * (1 + RUN * _U / (1 - RUN * _U) + m * 2.0 ** -53 / (1 - m * 2.0 ** -53)) - 1
    bl = torch.zeros(1, dtype=torch.float64, device=dev)
    bg = torch.zeros(p, dtype=torch.float64, device=dev)
    bH = torch.zeros((p, p), dtype=torch.float64, device=dev)
    ab = beta.double().abs()
    for i in range(0, n, _SPEC_ROWS):
        Z, yy, eta, mu, sp = _rows64(X, y, beta, i)
        A = Z.abs()
        e = gk * (A @ ab)
        d_res = e / 4 + 3 * _U + _U * (yy - mu).abs()
        d_om = e / (6 * math.sqrt(3)) + 4 * _U
        b = (1 + yy.abs()) * e * (1 + 2 * _U) + _U * (4 + (yy * eta).abs() + 2 * sp)
        bl += (b * (1 + G) + G * (yy * eta - sp).abs()).sum()
        bg += A.T @ (d_res * (1 + G) + G * (yy - mu).abs())
        bH += (A * (d_om * (1 + G) + G * mu * (1 - mu))[:, None]).T @ A
    zmax = max(1.0, float(X.abs().max())) if n else 1.0
    floor = 3 * n * 2.0 ** -126
    return bl + floor, bg + floor * zmax, bH + floor * zmax * zmax


# ---- float64 algebra on the statistics (plain torch on either device: the matrices are tiny) ----

def _unpenalised(p: int, like: torch.Tensor) -> torch.Tensor:
    """The diagonal of I': ones with a zero in the intercept's place."""
    e = torch.ones(p, dtype=torch.float64, device=like.device)
    e[-1] = 0.0
    return e


def penalised(ll: torch.Tensor, beta: torch.Tensor, l2: float = 0.0) -> float:
    """``ll - l2 / 2 sum_{c < d} beta_c^2``: what ``fit`` maximises."""
    b = beta.double()
    return float(ll[0]) - 0.5 * l2 * float((b[:-1] * b[:-1]).sum())


def newton_step(beta: torch.Tensor, ll: torch.Tensor, g: torch.Tensor, H: torch.Tensor, l2: float = 0.0):
    """``delta`` [p] (float64) of ``(H + l2 I') delta = g - l2 I' beta`` by Cholesky; ``I'`` is the identity
    with a zero in the intercept's place.  ``ll`` is not used by the step: the argument keeps the call
    ``newton_step(beta, *newton_stats(...))``."""
    e = _unpenalised(g.shape[0], g)
    A = H + l2 * torch.diag(e)
    rhs = g - l2 * e * beta.double()
    return torch.cholesky_solve(rhs[:, None], torch.linalg.cholesky(A))[:, 0]


def predict_proba(X: torch.Tensor, beta: torch.Tensor) -> torch.Tensor:
    """``sigmoid([X | 1] beta)`` (fp32 [n]).  A one-column matrix product: the vector form failed in
    the BLAS at 2^24 rows."""
    return torch.sigmoid(torch.mm(X, beta[:-1, None])[:, 0] + beta[-1])


class Newton:
    """The damped Newton iteration as a state machine, one ``update`` per pass over the data, so that
    ``fit`` and examples/LogisticRegression share the rule.  ``beta`` (fp32) is the point the next
    pass evaluates.  The float64 iterate is ``b``; a step goes from ``fl32(b)``, where the statistics
    were taken: ``b' = fl32(b) + step delta``.  A candidate whose penalised log-likelihood went DOWN is
    replaced by one at half the step (at most ``MAX_HALVINGS`` times, then taken as it is); an
    accepted one is recorded in ``history`` as ``{iter, ll, step, halvings}`` (iter 0: the start).  Done
    when the accepted move is ``max |b' - b| <= tol`` or after ``max_iters`` accepted steps."""

    def __init__(self, p: int, device, l2: float = 0.0, max_iters: int = 25, tol: float = 1e-8):
        self.l2, self.max_iters, self.tol = float(l2), int(max_iters), float(tol)
        self.b = torch.zeros(p, dtype=torch.float64, device=device)  # the last accepted iterate
        self.beta = self.b.float()
        self.pll = -math.inf
        self.base = self.delta = None  # the step under trial: cand = base + step delta
        self.step, self.halvings = 0.0, 0
        self.history: list = []

    def update(self, ll, g, H) -> bool:
        """Take the statistics at ``self.beta``; returns whether another pass is needed."""
        pll = penalised(ll, self.beta, self.l2)
        if self.delta is not None and pll < self.pll and self.halvings < MAX_HALVINGS:
            self.step, self.halvings = self.step / 2, self.halvings + 1
            self.beta = (self.base + self.step * self.delta).float()
            return True
        cand = self.b if self.delta is None else self.base + self.step * self.delta
        move = float((cand - self.b).abs().max())
        self.history.append({"iter": len(self.history), "ll": float(ll[0]), "step": self.step,
                             "halvings": self.halvings})
        started, self.b, self.pll = self.delta is not None, cand, pll
        if (started and move <= self.tol) or len(self.history) > self.max_iters:
            self.beta = self.b.float()
            return False
        self.base, self.delta = self.beta.double(), newton_step(self.beta, ll, g, H, self.l2)
        self.step, self.halvings = 1.0, 0
        self.beta = (self.base + self.delta).float()
        return True


def fit(X: torch.Tensor, y: torch.Tensor, l2: float = 0.0, max_iters: int = 25, tol: float = 1e-8):
    """``(beta fp32 [d + 1], history)``: the one-device driver, from ``beta = 0``.  One ``newton_stats``
    pass per trial point (see ``Newton``)."""
    st = Newton(X.shape[1] + 1, X.device, l2, max_iters, tol)
    while st.update(*newton_stats(X, y, st.beta.contiguous())):
        pass
    return st.beta, st.history
