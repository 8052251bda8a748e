"""The fused k-means map step (ops.kmeans.step, csrc/hip/kmeans.hip) against the
plain torch chain a user would write in device_mapfn (``X @ C.T`` + ``argmin`` +
``index_add_``, in row blocks of 2^20 so the n x k scores fit), on the same
tensors in the same process, alternating: n = 2^24 points, d in {16, 64, 128},
k in {16, 256, 1024}.  One step on a sample is validated against the CPU
specification first (labels under the margin rule, counts, sums, cost); a wrong
answer exits non-zero.  Times are medians of device-event timings after
warm-up; each shape also gets its two floors, 2 n k d FLOP at the fp32 MFMA
peak and 4 n d bytes at the HBM peak (datasheet: 157.3 TFLOP/s, 8 TB/s).

``--dtype bf16 [--terms T]`` measures the bf16 step (csrc/hip/kmeans_bf16.hip)
instead, by the same method.  Its partner is the fp32 ``ops.kmeans.step`` on the
same points widened to fp32 (the kernel the line above measures), and the
sample is validated against the CPU specification of the bf16 path (C_T,
u~ = 2^-23, E_i(T)).  Floors: 2 T n k d FLOP at the bf16 matrix peak
(datasheet: 2.5 PFLOP/s dense) and 2 n d bytes at the HBM peak.

``--op seed`` measures the k-means|| seeding path (csrc/hip/kmeans_seed.hip) at
the same shapes with m = 2k candidates (rows of X): one ``min_dist`` round from
fresh state against the torch chain ``(|x|^2 + |c|^2 - 2 X @ C.T).min(1)``
folded into ``mind`` in row blocks, and against ``ops.kmeans.assign`` at the
same (d, m), alternating; ``sample`` alone (its host read of the total
included); and Lloyd's iteration count and final cost from "rows" against
"kmeans||" seeds (``ops.kmeans.seed``, timed as a whole).  A sample of the
``min_dist`` result is validated against float64 with the bound B_i first.

    python tools/bench_kmeans.py [--n 16777216] [--steps 5] [--warmup 2] [--shapes 16x16,64x256]
                                 [--dtype bf16 [--terms 3]] [--op seed]
"""
import argparse
import json
import os
import statistics
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from lua_mapreduce_1_amd.ops import kmeans as K  # noqa: E402

PEAK_FLOPS = 157.3e12  # MI355X fp32 matrix
PEAK_BF16 = 2.5e15     # MI355X bf16 matrix, dense (datasheet, not measured here)
PEAK_BYTES = 8.0e12    # MI355X HBM3E
U = 2.0 ** -24


def make(n, d, k, dev):
    g = torch.Generator(device=dev).manual_seed(1)
    C = torch.randn(k, d, device=dev, generator=g) * 10
    X = torch.empty(n, d, device=dev)
    for i in range(0, n, 1 << 20):
        m = min(1 << 20, n - i)
        X[i:i + m] = C[torch.randint(0, k, (m,), device=dev, generator=g)] + torch.randn(m, d, device=dev, generator=g)
    return X, C


def torch_chain(X, C):
    k, d = C.shape
    sums = torch.zeros(k, d, device=X.device)
    counts = torch.zeros(k, dtype=torch.int64, device=X.device)
    cn = (C * C).sum(1)
    for i in range(0, X.shape[0], 1 << 20):
        x = X[i:i + (1 << 20)]
        lab = (cn - 2 * (x @ C.T)).argmin(1)
        sums.index_add_(0, lab, x)
        counts += torch.bincount(lab, minlength=k)
    return sums, counts


def validate(X, C, rows=4096, terms=3):
    """One kernel step on a strided sample against the CPU specification
    (bf16 points: against C_T, with the bf16 path's E_i(T))."""
    n, d = X.shape
    xs = X[::max(1, n // rows)][:rows].contiguous()
    sums, counts, cost, lab = K.step(xs, C, labels=True, terms=terms)
    s64, c64, q64, l64 = K.step(xs.cpu(), C.cpu(), labels=True, terms=terms)
    X64, C64 = xs.cpu().double(), K._spec_centroids(xs, C.cpu(), terms).double()
    D = torch.cdist(X64, C64) ** 2
    g = (d + 2) * U / (1 - (d + 2) * U)
    gl = g if X.dtype == torch.float32 else 2 * (terms * d + 2) * U / (1 - 2 * (terms * d + 2) * U)
    E = 2 * gl * (X64.norm(dim=1) + C64.norm(dim=1).max()) ** 2
    lab = lab.cpu().long()
    best = D.min(1).values
    ok = bool((D.gather(1, lab[:, None])[:, 0] <= best + E + 1e-9 * best).all())  # (1e-9: cdist's own rounding)
    two = D.topk(min(2, D.shape[1]), dim=1, largest=False).values
    clear = (two[:, -1] - two[:, 0] > E + 1e-9 * best) if D.shape[1] > 1 else torch.ones(len(lab), dtype=torch.bool)
    ok &= bool((lab[clear] == l64.long()[clear]).all())
    ok &= bool((counts.cpu() == torch.bincount(lab, minlength=C.shape[0])).all())
    want = torch.zeros_like(s64).index_add_(0, lab, X64)
    mass = torch.zeros_like(s64).index_add_(0, lab, X64.abs())
    nj = counts.cpu().double()
    ok &= bool(((sums.cpu() - want).abs() <= 2 * (nj * U / (1 - nj * U))[:, None] * mass).all())
    ok &= bool(abs(float(cost.cpu()) - float(q64)) <= float((E + g * X64.norm(dim=1) ** 2).sum()) + 1e-6 * float(q64))
    return ok


def timed(fn, steps, warmup):
    for _ in range(warmup):
        fn()
    out = []
    for _ in range(steps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        out.append(a.elapsed_time(b))
    return out


def bench_bf16(a, X, X32, C, box):
    """The bf16 step on X against the fp32 step on the same points widened to fp32; 1 if invalid."""
    n, (k, d) = a.n, C.shape
    X32.copy_(X)
    valid = validate(X, C, terms=a.terms)

    def acc():
        return (torch.zeros(k, d, dtype=torch.float64, device=X.device),
                torch.zeros(k, dtype=torch.int64, device=X.device), torch.zeros(1, dtype=torch.float64, device=X.device))
    ab, af = acc(), acc()
    tb, tf = [], []
    for _ in range(a.steps):  # alternate the two, one timed call each per round
        tb += timed(lambda: K.step(X, C, *ab, terms=a.terms), 1, a.warmup if not tb else 0)
        tf += timed(lambda: K.step(X32, C, *af), 1, a.warmup if not tf else 0)
    calls = a.steps + a.warmup
    valid &= int(ab[1].sum()) == calls * n
    # C_T and C may split near-ties differently: counts agree to within a 1e-3 share at T = 3
    valid &= a.terms < 3 or float((ab[1] - af[1]).abs().sum()) <= 1e-3 * n * calls
    ms_b, ms_f = statistics.median(tb), statistics.median(tf)
    f_flop, f_byte = 2.0 * a.terms * n * k * d / PEAK_BF16 * 1e3, 2.0 * n * d / PEAK_BYTES * 1e3
    print(json.dumps({"box": box, "dtype": "bf16", "terms": a.terms, "n": n, "d": d, "k": k, "valid": bool(valid),
                      "bf16_ms": round(ms_b, 3), "bf16_ms_all": [round(t, 3) for t in tb], "fp32_ms": round(ms_f, 3),
                      "fp32_ms_all": [round(t, 3) for t in tf], "fp32_over_bf16": round(ms_f / ms_b, 2),
                      "mfma_floor_ms": round(f_flop, 4), "hbm_floor_ms": round(f_byte, 3),
                      "mfma_fraction": round(f_flop / ms_b, 3), "hbm_fraction": round(f_byte / ms_b, 3)}), flush=True)
    return 0 if valid else 1


def lloyd(X, C, max_iters=20, tol=1e-4):
    """Lloyd's from C with ops.kmeans.step: (iterations, final cost)."""
    for it in range(1, max_iters + 1):
        sums, counts, cost, _ = K.step(X, C)
        new = torch.where((counts > 0)[:, None], sums / counts.clamp(min=1)[:, None], C.double())
        shift = float(((new - C.double()) ** 2).sum(1).max())
        C = new.float().contiguous()
        if shift <= tol:
            break
    return it, float(cost)


def bench_seed(a, X, box, d, k):
    """One min_dist round against the torch chain and against assign, sample alone, Lloyd's from both inits."""
    n, m, dev = a.n, 2 * k, X.device
    g = torch.Generator(device=dev).manual_seed(2)
    Cm = X[torch.randint(0, n, (m,), device=dev, generator=g)].contiguous()
    xs = X[::max(1, n // 4096)][:4096].contiguous()  # validation: a sample against float64, bound B_i
    md, _nr, ph = K.min_dist(xs, Cm)
    X64, C64 = xs.cpu().double(), Cm.cpu().double()
    D = (torch.cdist(X64, C64) ** 2).min(1).values
    gm = (d + 2) * U / (1 - (d + 2) * U)
    E = 2 * gm * (X64.norm(dim=1) + C64.norm(dim=1).max()) ** 2
    B = E + gm * X64.norm(dim=1) ** 2 + 2 * U * (D + E)
    valid = bool(((md.cpu().double() - D).abs() <= B + 1e-9 * D).all())  # (1e-9: cdist's own rounding)
    valid &= abs(float(ph) - float(md.double().sum())) <= 1e-12 * float(ph)

    mind = torch.empty(n, device=dev)
    near = torch.empty(n, dtype=torch.int32, device=dev)
    tmind = torch.empty(n, device=dev)
    blk = 1 << (20 if m <= 1024 else 19)

    def kernel():
        K.min_dist(X, Cm, mind, near)

    def chain():
        cn = (Cm * Cm).sum(1)
        for i in range(0, n, blk):
            x = X[i:i + blk]
            d2 = ((x * x).sum(1)[:, None] + cn - 2 * (x @ Cm.T)).min(1).values
            torch.minimum(tmind[i:i + blk], d2.clamp_(min=0), out=tmind[i:i + blk])

    tk, tt, ta = [], [], []
    for _ in range(a.steps):  # alternate the three, one timed call each per round, from fresh state
        for buf, fn, out in ((mind, kernel, tk), (tmind, chain, tt), (None, lambda: K.assign(X, Cm), ta)):
            for _w in range(a.warmup if not out else 0):
                fn()
            if buf is not None:
                buf.fill_(float("inf"))
            out += timed(fn, 1, 0)
    # the full-size result against the chain: either side is within E_i + gamma_{d+2} |x_i|^2 + 2 u dist of the
    # truth (a dot product of d terms errs by at most gamma_d |x| |c| in any order)
    xn = torch.cat([(X[i:i + blk] ** 2).sum(1) for i in range(0, n, blk)])
    tol = 2 * (2 * gm * (xn.sqrt() + float(Cm.norm(dim=1).max())) ** 2 + gm * xn + 2 * U * tmind)
    agrees = bool(((mind - tmind).abs() <= tol).all())
    _m, _n, phi = K.min_dist(X, Cm, mind, near)
    ts = timed(lambda: K.sample(X, mind, phi, float(m), 1, 0), a.steps, a.warmup)
    picked = len(K.sample(X, mind, phi, float(m), 1, 0)[0])

    rows0 = X[torch.from_numpy(np.random.default_rng(1).choice(n, k, replace=False)).to(dev)].contiguous()
    t0 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t0[0].record()
    seeds, info = K.seed(X, k, seed=1)
    t0[1].record()
    t0[1].synchronize()
    it_r, cost_r = lloyd(X, rows0)
    it_s, cost_s = lloyd(X, seeds)
    ms_k, ms_t, ms_a = statistics.median(tk), statistics.median(tt), statistics.median(ta)
    f_flop, f_byte = 2.0 * n * m * d / PEAK_FLOPS * 1e3, (4.0 * n * d + 12.0 * n) / PEAK_BYTES * 1e3
    print(json.dumps({"box": box, "op": "seed", "n": n, "d": d, "k": k, "m": m, "valid": bool(valid),
                      "agrees_with_torch": agrees, "min_dist_ms": round(ms_k, 3), "min_dist_ms_all": [round(t, 3) for t in tk],
                      "torch_ms": round(ms_t, 3), "torch_over_min_dist": round(ms_t / ms_k, 2),
                      "assign_ms": round(ms_a, 3), "assign_ms_all": [round(t, 3) for t in ta],
                      "assign_over_min_dist": round(ms_a / ms_k, 3), "mfma_floor_ms": round(f_flop, 3),
                      "hbm_floor_ms": round(f_byte, 3), "sample_ms": round(statistics.median(ts), 3),
                      "sample_ms_all": [round(t, 3) for t in ts], "sample_picked": picked,
                      "seed_total_ms": round(t0[0].elapsed_time(t0[1]), 1), "seed_candidates": len(info["candidates"]),
                      "lloyd_rows": {"iters": it_r, "cost": cost_r}, "lloyd_kmeans||": {"iters": it_s, "cost": cost_s}}),
          flush=True)
    return 0 if valid and agrees else 1


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=1 << 24)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--shapes", default=",".join(f"{d}x{k}" for d in (16, 64, 128) for k in (16, 256, 1024)))
    ap.add_argument("--dtype", choices=("fp32", "bf16"), default="fp32")
    ap.add_argument("--terms", type=int, default=3)
    ap.add_argument("--op", choices=("step", "seed"), default="step")
    a = ap.parse_args()
    if a.dtype == "fp32" and a.terms != 3:
        ap.error("--terms goes with --dtype bf16")
    if not torch.cuda.is_available():
        sys.exit("bench_kmeans needs a GPU: nothing is measured without one")
    dev = torch.device("cuda", 0)
    box = torch.cuda.get_device_name(0)
    bad = 0
    for shape in a.shapes.split(","):
        d, k = (int(v) for v in shape.split("x"))
        X, C = make(a.n, d, k, dev)
        if a.op == "seed":
            bad += bench_seed(a, X, box, d, k)
            del X, C
            continue
        if a.dtype == "bf16":
            bad += bench_bf16(a, X.to(torch.bfloat16), X, C, box)
            del X, C
            continue
        valid = validate(X, C)
        sums = torch.zeros(k, d, dtype=torch.float64, device=dev)
        counts = torch.zeros(k, dtype=torch.int64, device=dev)
        cost = torch.zeros(1, dtype=torch.float64, device=dev)
        tk, tt = [], []
        for _ in range(a.steps):  # alternate the two, one timed call each per round
            tk += timed(lambda: K.step(X, C, sums, counts, cost), 1, a.warmup if not tk else 0)
            tt += timed(lambda: torch_chain(X, C), 1, a.warmup if not tt else 0)
        _s, tcounts = torch_chain(X, C)
        calls = a.steps + a.warmup
        valid &= int(counts.sum()) == calls * a.n
        # the two paths may split near-ties differently: counts agree to within a 1e-3 share
        valid &= float((counts.double() / calls - tcounts.double()).abs().sum()) <= 1e-3 * a.n
        ms_k, ms_t = statistics.median(tk), statistics.median(tt)
        f_flop, f_byte = 2.0 * a.n * k * d / PEAK_FLOPS * 1e3, 4.0 * a.n * d / PEAK_BYTES * 1e3
        print(json.dumps({"box": box, "n": a.n, "d": d, "k": k, "valid": bool(valid), "kernel_ms": round(ms_k, 3),
                          "kernel_ms_all": [round(t, 3) for t in tk], "torch_ms": round(ms_t, 3),
                          "torch_over_kernel": round(ms_t / ms_k, 2), "mfma_floor_ms": round(f_flop, 3),
                          "hbm_floor_ms": round(f_byte, 3), "mfma_fraction": round(f_flop / ms_k, 3),
                          "hbm_fraction": round(f_byte / ms_k, 3)}), flush=True)
        bad += not valid
        del X, C
    sys.exit(1 if bad else 0)


if __name__ == "__main__":
    main()
