"""Lloyd's k-means as an iterative MapReduce job on the tensor plane.

One module provides every function (pass it as taskfn, mapfn, partitionfn,
reducefn and finalfn) and runs in SPMD form only, through ``execute_spmd.py`` /
``lua_mapreduce_1_amd.spmd``.  A server/worker form would need the model in a
persistent table and the blob store, as examples/DigitsMLP has; that is out of
scope here.

* ``init(args)``: ``files`` — raw little-endian fp32 ``[n_i, dim]`` row-major
  files, one per map job, or ``"synthetic"`` (``make_points(seed, n, dim, k,
  nsplits)``, with ``n`` and ``nsplits`` in the args) — ``k``, ``dim``,
  ``max_iters`` (20), ``tol`` (1e-4: stop when the largest squared centroid
  shift is <= tol), ``seed``, and optionally ``centroids`` (array or raw fp32
  file).  Without ``centroids`` every rank picks the same k distinct rows,
  ``default_rng(seed).choice(n_total, k, replace=False)``, and reads just those
  rows through a memmap.  ``point_dtype`` is ``"fp32"`` (default) or
  ``"bf16"``: the files are then raw little-endian bf16 rows, ``"synthetic"``
  points are rounded to bf16 once, the step runs on the 16-bit matrix cores
  against ``terms`` (3) bf16 pieces of every centroid (ops/kmeans.py), and the
  centroids stay fp32.  numpy has no bf16: on the host such rows are
  ``uint16`` and are widened by a 16-bit shift where values are needed.
* map: one job per file.  The job's points go to the device once and stay
  there across iterations; ``ops.kmeans.step`` (one fused MFMA launch on a
  GPU) assigns them to the replicated centroids and its partial sums are
  ADDED into the tensor plane's accumulators (a rank may run several jobs).
* the plane is fp32: ``SUMS`` [k*dim] carries fp32 of the float64 partial
  sums, ``COST`` [1] the cost, and ``COUNTS`` [2k] every cluster's count as two
  exact fp32 words, ``c & 0xFFFFF`` and ``c >> 20`` (exact for W <= 16 ranks
  and 2^44 points); ``device_finalfn`` rejoins them in int64.
* final (every rank): centroid = sum / count, an empty cluster keeps its
  centroid; ``HISTORY`` gets ``{iter, cost, shift, empty}``; ``"loop"`` until
  the shift is <= tol or ``max_iters`` is reached.  Afterwards ``CENTROIDS``
  (device tensor) and ``predict(X)`` (``ops.kmeans.assign``) serve the model.
* ``init_method``: ``"rows"`` (default: the k random rows above) or
  ``"kmeans||"`` (Bahmani et al., "Scalable K-Means++"), with ``seed_ell``
  (2k: the expected picks of a round) and ``seed_rounds`` (5).  The first
  engine iterations are then seeding rounds, a phase of the module state: the
  map runs ``ops.kmeans.min_dist`` (csrc/hip/kmeans_seed.hip) on the job's
  resident points against the replicated newest batch of candidates, keeps
  ``mind`` / ``near`` per job beside the points and adds ``phi`` into ``COST``;
  the final, on every rank, runs ``ops.kmeans.sample`` over its own jobs with
  the job's global row offset (the selection does not depend on how the points
  are split), exchanges the picks with ``all_gather_object``, orders them by
  global index and appends them to the candidates.  One more iteration folds
  the last batch, the per-job ``bincount(near)`` are summed across ranks, and
  every rank sets ``CENTROIDS = ops.kmeans.recluster(...)`` with the same seed.
  Lloyd's then proceeds as above: ``HISTORY`` and ``max_iters`` count Lloyd
  iterations only; the seeding rounds go to ``SEED_HISTORY`` (``{round, phi,
  candidates}``) and ``SEED_INFO`` (``indices`` per round, ``candidates``,
  ``weights``, ``seeds``).  Seeding rounds are not checkpointed.
* ``naive(splits, ...)``: plain float64 numpy Lloyd's with the same init, tie
  rule, empty-cluster rule and stopping rule; with ``init_method="kmeans||"``
  the same seeding in float64 with the same hash and rule, and the result also
  holds ``seed_indices`` (per round) and ``seed_margin``: for every point the
  smallest relative distance ``|u phi - ell' mind| / (ell' mind)`` of the rule's
  two sides over the rounds (ell' = ell 2^24), i.e. how far the selection is
  from depending on rounding.
"""
from __future__ import annotations

import numpy as np
import torch

from lua_mapreduce_1_amd.ops import io as _io
from lua_mapreduce_1_amd.ops import kmeans as K
from lua_mapreduce_1_amd.parallel import dist as D

NUM_REDUCERS = 10
KEYS = ("SUMS", "COUNTS", "COST")
_LO_BITS = 20

device_reduce = "tensor_sum"
spmd_replicated_taskfn = True

HISTORY: list = []
SEED_HISTORY: list = []
SEED_INFO: dict = {}
CENTROIDS = None
_st: dict = {}


def make_points(seed: int, n: int, dim: int, k: int, nsplits: int) -> list:
    """``nsplits`` fp32 arrays [n_i, dim]: n points around k Gaussian blobs
    (centres N(0, 10^2), unit spread), in random order."""
    rng = np.random.default_rng(seed)
    centres = rng.normal(0.0, 10.0, (k, dim))
    pts = centres[rng.integers(0, k, n)] + rng.normal(0.0, 1.0, (n, dim))
    return [np.ascontiguousarray(s, dtype=np.float32) for s in np.array_split(pts, nsplits)]


def to_bf16(a: np.ndarray) -> np.ndarray:
    """fp32 array -> its bf16 round-to-nearest-even, as uint16."""
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).to(torch.bfloat16).view(torch.int16).numpy() \
        .view(np.uint16)


def widen(a: np.ndarray) -> np.ndarray:
    """bf16 rows held as uint16 -> the same values in fp32 (exact)."""
    return (np.asarray(a).astype(np.uint32) << 16).view(np.float32)


def _rows(src, dim: int, point_dtype: str = "fp32") -> np.ndarray:
    """A split as a [n_i, dim] array (a memmap of a file): fp32, or uint16 for bf16 points."""
    if isinstance(src, np.ndarray):
        return src
    return np.memmap(src, dtype="<u2" if point_dtype == "bf16" else "<f4", mode="r").reshape(-1, dim)


def _values(rows: np.ndarray) -> np.ndarray:
    return widen(rows) if rows.dtype == np.uint16 else rows


def take_rows(splits, pick, dim: int, point_dtype: str = "fp32") -> np.ndarray:
    """Rows ``pick`` (global indices) of the concatenated splits, fp32."""
    splits = [_rows(s, dim, point_dtype) for s in splits]
    sizes = [s.shape[0] for s in splits]
    ends = np.cumsum(sizes)
    out = np.empty((len(pick), dim), dtype=np.float32)
    for j, r in enumerate(pick):
        s = int(np.searchsorted(ends, r, side="right"))
        out[j] = _values(splits[s][r - (ends[s] - sizes[s])])
    return out


def initial_centroids(splits, k: int, dim: int, seed: int, point_dtype: str = "fp32") -> np.ndarray:
    """k distinct rows of the concatenated splits, the same on every rank."""
    total = sum(_rows(s, dim, point_dtype).shape[0] for s in splits)
    return take_rows(splits, np.random.default_rng(seed).choice(int(total), k, replace=False), dim, point_dtype)


def split_counts(c: torch.Tensor) -> torch.Tensor:
    """int64 counts [k] -> fp32 [2k]: the low 20 bits, then the rest."""
    return torch.cat([(c & ((1 << _LO_BITS) - 1)), (c >> _LO_BITS)]).to(torch.float32)


def rejoin_counts(t: torch.Tensor) -> torch.Tensor:
    """fp32 [2k] (sums of split words) -> int64 counts [k]."""
    k = t.numel() // 2
    w = t.to(torch.int64)
    return w[:k] + (w[k:] << _LO_BITS)


def init(args):
    global HISTORY, SEED_HISTORY, SEED_INFO, CENTROIDS
    a = dict(args or {})
    _st.clear()
    HISTORY, SEED_HISTORY, SEED_INFO = [], [], {}
    CENTROIDS = None
    k, dim = int(a["k"]), int(a["dim"])
    files = a.get("files", "synthetic")
    seed = int(a.get("seed", 0))
    dt, terms = a.get("point_dtype", "fp32"), int(a.get("terms", 3))
    if dt not in ("fp32", "bf16"):
        raise ValueError(f"KMeans: point_dtype is 'fp32' or 'bf16' (got {dt!r})")
    if files == "synthetic":
        splits = make_points(seed, int(a.get("n", 20000)), dim, k, int(a.get("nsplits", 4)))
        if dt == "bf16":
            splits = [to_bf16(s) for s in splits]
    else:
        splits = [files] if isinstance(files, str) else list(files)
    c = a.get("centroids")
    method = a.get("init_method", "rows")
    if method not in ("rows", "kmeans||"):
        raise ValueError(f"KMeans: init_method is 'rows' or 'kmeans||' (got {method!r})")
    seeding = None
    if method == "kmeans||":
        if c is not None:
            raise ValueError("KMeans: init_method 'kmeans||' and centroids exclude each other")
        sizes = [_rows(s, dim, dt).shape[0] for s in splits]
        first = np.array([np.random.default_rng(seed).integers(int(sum(sizes)))], dtype=np.int64)
        seeding = dict(ell=float(a.get("seed_ell", 2 * k)), rounds=int(a.get("seed_rounds", 5)), total=0, jobs={},
                       offsets=[int(o) for o in np.cumsum([0] + sizes[:-1])], indices=[first],
                       batches=[take_rows(splits, first, dim, dt)])
        c0 = np.zeros((k, dim), dtype=np.float32)  # never read: the seeding sets CENTROIDS
    elif c is None:
        c0 = initial_centroids(splits, k, dim, seed, dt)
    elif isinstance(c, str):
        c0 = np.fromfile(c, dtype="<f4").reshape(k, dim)
    else:
        c0 = np.asarray(c, dtype=np.float32).reshape(k, dim)
    _st.update(k=k, dim=dim, splits=splits, c0=np.ascontiguousarray(c0, dtype=np.float32), points={},
               max_iters=int(a.get("max_iters", 20)), tol=float(a.get("tol", 1e-4)), bf16=dt == "bf16", terms=terms,
               seed=seed, seeding=seeding)


def taskfn(emit):
    for j, s in enumerate(_st["splits"]):
        emit(j + 1, j if isinstance(s, np.ndarray) else s)


def device_tensor_layout() -> dict:
    return {"SUMS": _st["k"] * _st["dim"], "COUNTS": 2 * _st["k"], "COST": 1}


def _centroids(device) -> torch.Tensor:
    global CENTROIDS
    if CENTROIDS is None:
        CENTROIDS = torch.from_numpy(_st["c0"]).to(device)
    return CENTROIDS


def _tdtype():
    return torch.bfloat16 if _st["bf16"] else torch.float32


def _tensor(rows: np.ndarray) -> torch.Tensor:
    """A host array of points as a tensor of the job's point dtype (uint16 rows are bf16 bits)."""
    if rows.dtype == np.uint16:
        return torch.from_numpy(np.ascontiguousarray(rows).view(np.int16)).view(torch.bfloat16)
    return torch.from_numpy(np.ascontiguousarray(rows, dtype=np.float32)).to(_tdtype())


def _points(key, value, device) -> torch.Tensor:
    x = _st["points"].get(key)
    if x is None:
        if isinstance(value, str):
            x = _io.load_file(value, device).view(_tdtype()).view(-1, _st["dim"])
        else:
            x = _tensor(_st["splits"][int(value)]).to(device)
        _st["points"][key] = x
    return x


def device_mapfn(key, value, emit):
    """Assign the job's points (device-resident after the first iteration) to
    the replicated centroids and add the partial sums into the plane."""
    dev = emit.device
    if _st["seeding"] is not None:
        return _seed_map(key, _points(key, value, dev), emit)
    sums, counts, cost, _ = K.step(_points(key, value, dev), _centroids(dev), terms=_st["terms"])
    emit.accumulator("SUMS").add_(sums.reshape(-1).to(torch.float32))
    cw = emit.accumulator("COUNTS")
    cw.copy_(split_counts(rejoin_counts(cw) + counts))  # add, then renormalise the two words
    emit.accumulator("COST").add_(cost.to(torch.float32))


def _seed_map(key, x, emit):
    """A seeding round's map: fold the newest batch of candidates into the job's mind / near."""
    sd = _st["seeding"]
    batch = torch.from_numpy(sd["batches"][-1]).to(x.device)
    mind, near = sd["jobs"].get(key, (None, None))
    for i in range(0, len(batch), K.MAX_M):  # a batch beyond the kernel's range goes in pieces
        mind, near, phi = K.min_dist(x, batch[i:i + K.MAX_M].contiguous(), mind, near, base=sd["total"] + i)
    sd["jobs"][key] = (mind, near)
    emit.accumulator("COST").add_(phi.to(torch.float32))


def _seed_final(res, engine):
    """A seeding round's final, on every rank: sample the next batch, or, after
    the last fold, weigh the candidates and pick the k seeds."""
    global CENTROIDS
    sd = _st["seeding"]
    phi = float(res.tensors["COST"][0])
    sd["total"] += len(sd["batches"][-1])
    t = len(SEED_HISTORY)
    picked = 0
    if t < sd["rounds"]:
        mine = []
        for key, (mind, _near) in sd["jobs"].items():
            idx, rows = K.sample(_st["points"][key], mind, phi, sd["ell"], _st["seed"], t,
                                 offset=sd["offsets"][int(key) - 1])
            mine.append((idx.cpu().numpy(), rows.cpu().numpy()))
        got = [p for r in D.all_gather_object(mine, engine.group) for p in r]
        idx = np.concatenate([p[0] for p in got]) if got else np.zeros(0, dtype=np.int64)
        order = np.argsort(idx, kind="stable")
        picked = len(idx)
        if picked:
            sd["indices"].append(idx[order])
            sd["batches"].append(np.concatenate([p[1] for p in got])[order])
    SEED_HISTORY.append({"round": t + 1, "phi": phi, "candidates": sd["total"] + picked})
    if engine.rank == 0 and engine.verbose:
        print("# kmeans|| round %(round)d phi %(phi).6g candidates %(candidates)d" % SEED_HISTORY[-1], flush=True)
    if picked:
        return "loop"  # the next iteration folds the new batch
    mine = sum(torch.bincount(near.long(), minlength=sd["total"]).cpu().numpy() for _m, near in sd["jobs"].values())
    weights = sum(D.all_gather_object(mine, engine.group))
    cands = np.concatenate(sd["batches"])
    CENTROIDS = K.recluster(cands, weights, _st["k"], _st["seed"]).to(engine.device)
    SEED_INFO.update(indices=sd["indices"], candidates=cands, weights=np.asarray(weights),
                     seeds=CENTROIDS.cpu().numpy())
    _st["seeding"] = None
    return "loop"


def partitionfn(key):
    return sum(key.encode()) % NUM_REDUCERS


def reducefn(key, values, emit):
    emit(sum(np.asarray(v, dtype=np.float64) for v in values))


def device_finalfn(res, engine):
    """Every rank: move the centroids, record the iteration, decide to loop."""
    global CENTROIDS
    if _st["seeding"] is not None:
        return _seed_final(res, engine)
    k, dim = _st["k"], _st["dim"]
    old = _centroids(engine.device)
    counts = rejoin_counts(res.tensors["COUNTS"])
    sums = res.tensors["SUMS"].view(k, dim).to(torch.float64)
    live = counts > 0
    new = torch.where(live[:, None], sums / counts.clamp(min=1)[:, None].to(torch.float64), old.to(torch.float64))
    shift = float(((new - old.to(torch.float64)) ** 2).sum(1).max())
    CENTROIDS = new.to(torch.float32).contiguous()
    HISTORY.append({"iter": len(HISTORY) + 1, "cost": float(res.tensors["COST"][0]), "shift": shift,
                    "empty": int((~live).sum())})
    if engine.rank == 0 and engine.verbose:
        print("# kmeans iter %(iter)d cost %(cost).6g shift %(shift).3g empty %(empty)d" % HISTORY[-1], flush=True)
    return "loop" if shift > _st["tol"] and len(HISTORY) < _st["max_iters"] else True


def finalfn(pairs):
    raise RuntimeError("examples/KMeans runs in SPMD form only (device_finalfn)")


def mapfn(key, value, emit):
    raise RuntimeError("examples/KMeans runs in SPMD form only (device_mapfn)")


def predict(X) -> torch.Tensor:
    """int32 labels of the rows of X under the fitted centroids."""
    x = _tensor(X) if isinstance(X, np.ndarray) else torch.as_tensor(X).to(_tdtype())
    return K.assign(x.to(CENTROIDS.device).contiguous(), CENTROIDS, terms=_st["terms"])


def _naive_seed(X: np.ndarray, k: int, ell: float, rounds: int, seed: int) -> dict:
    """k-means|| in float64 numpy, round for round as the job runs it."""
    n = len(X)
    g = np.arange(n, dtype=np.uint64)
    indices = [np.array([np.random.default_rng(seed).integers(n)], dtype=np.int64)]
    mind, near, total, margin = np.full(n, np.inf), np.full(n, -1, dtype=np.int64), 0, np.full(n, np.inf)
    for t in range(rounds + 1):
        B = X[indices[-1]]
        for i in range(0, n, 8192):
            Dm = ((X[i:i + 8192, None, :] - B[None]) ** 2).sum(-1)
            j = Dm.argmin(1)
            take = Dm[np.arange(len(j)), j] < mind[i:i + 8192]
            mind[i:i + 8192][take] = Dm[np.arange(len(j)), j][take]
            near[i:i + 8192][take] = total + j[take]
        total += len(B)
        phi = float(mind.sum())
        if t == rounds:
            break
        lhs, rhs = K._u24(seed, t, g).astype(np.float64) * phi, ell * 2.0 ** 24 * mind
        margin = np.minimum(margin, np.where(rhs > 0, np.abs(lhs - rhs) / np.where(rhs > 0, rhs, 1.0), np.inf))
        pick = np.flatnonzero(K.selected(mind, phi, ell, seed, t, g))
        if len(pick) == 0:
            break
        indices.append(pick)
    weights = np.bincount(near, minlength=total)
    C = K.recluster(X[np.concatenate(indices)].astype(np.float32), weights, k, seed).numpy()
    return {"centroids": C, "seed_indices": indices, "seed_margin": margin, "seed_weights": weights}


def naive(splits, k: int, dim: int, max_iters: int = 20, tol: float = 1e-4, seed: int = 0, centroids=None,
          point_dtype: str = "fp32", init_method: str = "rows", seed_ell=None, seed_rounds: int = 5) -> dict:
    """Plain float64 numpy Lloyd's: the oracle of the job above (bf16 points:
    uint16 rows or bf16 files, i.e. the rounded points the job itself sees)."""
    X = np.concatenate([_values(np.asarray(_rows(s, dim, point_dtype))) for s in splits]).astype(np.float64)
    extra = {}
    if init_method == "kmeans||" and centroids is None:
        extra = _naive_seed(X, k, float(2 * k if seed_ell is None else seed_ell), seed_rounds, seed)
        centroids = extra.pop("centroids")
    C = (initial_centroids(splits, k, dim, seed, point_dtype) if centroids is None
         else np.asarray(centroids, dtype=np.float32).reshape(k, dim)).astype(np.float64)
    history = []
    while True:
        lab = np.empty(len(X), dtype=np.int64)
        cost = 0.0
        for i in range(0, len(X), 8192):
            D = ((X[i:i + 8192, None, :] - C[None]) ** 2).sum(-1)
            lab[i:i + 8192] = D.argmin(1)  # first minimum: the lowest index
            cost += float(D.min(1).sum())
        sums = np.zeros((k, dim))
        np.add.at(sums, lab, X)
        counts = np.bincount(lab, minlength=k)
        new = np.where(counts[:, None] > 0, sums / np.maximum(counts, 1)[:, None], C)
        shift = float(((new - C) ** 2).sum(1).max())
        C = new
        history.append({"iter": len(history) + 1, "cost": cost, "shift": shift, "empty": int((counts == 0).sum())})
        if not (shift > tol and len(history) < max_iters):
            return {"centroids": C, "history": history, **extra}
