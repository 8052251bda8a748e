"""The fused k-nearest-neighbour search (ops.knn.search, csrc/hip/knn.hip)
against two partners on the same operands in the same process, alternating: the
chunked torch chain a user would write (``|x|^2 - 2 Q X^T`` by ``addmm`` in
blocks, ``topk`` of every block, ``topk`` of the running candidates), and, at
K = 1, ``ops.kmeans.min_dist`` with the queries as its points and X folded in
as batches of 16384 candidates, the nearest thing the project had.  n = 2^24
standard-normal points, d in {16, 64, 128}, q in {1024, 16384}, K in {1, 16,
64}, plus one adversarial row: X sorted by descending distance to the first
query, so that query passes its threshold at every point.  A sample (64
queries, the first 65536 points) is validated against float64 within the
contract of ops/knn.py first, and the full result must agree with the torch
chain's neighbour sets on 99 % of the slots; a wrong answer exits non-zero.
Times are medians of device-event timings after warm-up.  Each shape also gets
the fp32 MFMA floor of its 2 q n d FLOP (datasheet: 157.3 TFLOP/s, not measured
here).

    python tools/bench_knn.py [--n 16777216] [--steps 3] [--warmup 1] [--shapes 16x1024x16,...]
"""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from lua_mapreduce_1_amd.ops import kmeans as K  # noqa: E402
from lua_mapreduce_1_amd.ops import knn as N  # noqa: E402

PEAK_FLOPS = 157.3e12  # MI355X fp32 matrix (datasheet)
U = 2.0 ** -24


def torch_chain(Q, X, k, qb=2048, xb=1 << 19):
    q, n = Q.shape[0], X.shape[0]
    dist = torch.empty((q, k), device=Q.device)
    idx = torch.empty((q, k), dtype=torch.int64, device=Q.device)
    for i in range(0, q, qb):
        Qb = Q[i:i + qb]
        bd = bi = None
        for j in range(0, n, xb):
            Xb = X[j:j + xb]
            S = torch.addmm((Xb * Xb).sum(1)[None], Qb, Xb.T, alpha=-2.0)
            v, o = S.topk(min(k, len(Xb)), dim=1, largest=False)
            bd, bi = (v, o + j) if bd is None else (torch.cat([bd, v], 1), torch.cat([bi, o + j], 1))
            if bd.shape[1] > k:
                bd, o = bd.topk(k, dim=1, largest=False)
                bi = bi.gather(1, o)
        dist[i:i + qb], idx[i:i + qb] = (bd + (Qb * Qb).sum(1)[:, None]).clamp_(min=0), bi
    return dist, idx


def min_dist_chain(Q, X):
    mind = near = None
    for j in range(0, X.shape[0], K.MAX_M):
        mind, near, _phi = K.min_dist(Q, X[j:j + K.MAX_M], mind, near, base=j)
    return mind, near


def validate(Q, X, k, rows=64, cols=1 << 16):
    """search on a sample against float64: ``(ok, worst error / B_i)`` over accuracy and separation."""
    qs, xs = Q[:rows].contiguous(), X[:cols].contiguous()
    dist, idx = N.search(qs, xs, k)
    d = Q.shape[1]
    D = torch.cdist(qs.double(), xs.double(), compute_mode="donot_use_mm_for_euclid_dist") ** 2
    g = (d + 2) * U / (1 - (d + 2) * U)
    qn2 = (qs.double() ** 2).sum(1)
    E = 2 * g * (qn2.sqrt() + (xs.double() ** 2).sum(1).max().sqrt()) ** 2
    B0 = E + g * qn2 + 2 * U * E
    Dg = D.gather(1, idx)
    share = ((dist.double() - Dg).abs() / (B0[:, None] + 2 * U * Dg)).max()
    rest = D.scatter(1, idx, float("inf")).min(1).values
    ok = bool(share <= 1) and bool((Dg.max(1).values <= rest + 2 * (B0 + 2 * U * D.max(1).values)).all())
    ok &= bool((idx.sort(1).values.diff(dim=1) > 0).all()) if k > 1 else True
    return ok, float(share)


def timed(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    out = fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b), out


def agreement(idx, tidx):
    """Share of the slots of ``idx`` whose index the torch chain also returned for that query."""
    return float((idx[:, :, None] == tidx[:, None, :]).any(2).float().mean())


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=1 << 24)
    ap.add_argument("--steps", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--shapes", default=",".join(f"{d}x{q}x{k}" for d in (16, 64, 128) for q in (1024, 16384)
                                                 for k in (1, 16, 64)) + ",16x1024x64xsorted")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("bench_knn needs a GPU: nothing is measured without one")
    dev = torch.device("cuda", 0)
    box = torch.cuda.get_device_name(0)
    bad, made = 0, None
    for shape in a.shapes.split(","):
        parts = shape.split("x")
        d, q, k = (int(v) for v in parts[:3])
        sorted_x = parts[3:] == ["sorted"]
        if made != (d, sorted_x):
            X = Q = None
            g = torch.Generator(device=dev).manual_seed(1)
            X = torch.randn(a.n, d, device=dev, generator=g)
            Qall = torch.randn(16384, d, device=dev, generator=g)
            if sorted_x:  # descending distance to the first query
                X = X[((X - Qall[0]) ** 2).sum(1).argsort(descending=True)].contiguous()
            made = (d, sorted_x)
        Q = Qall[:q].contiguous()
        valid, share = validate(Q, X, k)
        fns = {"knn": lambda: N.search(Q, X, k), "torch": lambda: torch_chain(Q, X, k)}
        if k == 1:
            fns["min_dist"] = lambda: min_dist_chain(Q, X)
        times, out = {name: [] for name in fns}, {}
        for name, fn in fns.items():
            for _ in range(a.warmup):
                fn()
        for _ in range(a.steps):  # alternate the partners, one timed call each per round
            for name, fn in fns.items():
                t, out[name] = timed(fn)
                times[name].append(t)
        agree = agreement(out["knn"][1], out["torch"][1])
        valid &= agree >= 0.99
        ms = {name: statistics.median(t) for name, t in times.items()}
        floor = 2.0 * q * a.n * d / PEAK_FLOPS * 1e3
        row = {"box": box, "n": a.n, "d": d, "q": q, "k": k, "sorted": sorted_x, "valid": bool(valid),
               "worst_error_over_B": round(share, 4), "torch_agreement": round(agree, 5),
               "slabs": N.default_slabs(q, a.n, dev), "knn_ms": round(ms["knn"], 3),
               "knn_ms_all": [round(t, 3) for t in times["knn"]], "torch_ms": round(ms["torch"], 3),
               "torch_over_knn": round(ms["torch"] / ms["knn"], 2), "mfma_floor_ms": round(floor, 3),
               "mfma_fraction": round(floor / ms["knn"], 3)}
        if k == 1:
            same = float((out["knn"][1][:, 0] == out["min_dist"][1]).float().mean())
            row.update(min_dist_ms=round(ms["min_dist"], 3), min_dist_over_knn=round(ms["min_dist"] / ms["knn"], 2),
                       min_dist_same_neighbour=round(same, 5))
        print(json.dumps(row), flush=True)
        bad += not valid
    sys.exit(1 if bad else 0)


if __name__ == "__main__":
    main()
