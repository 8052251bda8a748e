"""The fused moments kernel (ops.gram.moments, csrc/hip/gram.hip) against what a
user would write in torch, on the same operands in the same process,
alternating: (a) ``X.T @ X`` and ``X.sum(0)`` in fp32, and (b) the same in
float64 on a chunked upcast (2^20 rows at a time).  n = 2^24 points around a
common offset of 100 (shifted by a rough mean for ops.gram), d in {16, 64, 128,
256}, t = 0.  A sample (the first 2^18 rows) is first held to the contract of
ops/gram.py against float64, and the worst error is reported as a fraction of
the bound; a wrong answer exits non-zero.  Times are medians of device-event
timings after warm-up.  Each shape also gets two floors from the datasheet
(not measured here): reading X once at 8 TB/s, and n w^2 / 2 multiply-adds of
the upper triangle at 157.3 TFLOP/s of fp32 MFMA.

    python tools/bench_gram.py [--n 16777216] [--steps 3] [--warmup 1] [--dims 16,64,128,256]
"""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from lua_mapreduce_1_amd.ops import gram as Gm  # noqa: E402

PEAK_FLOPS = 157.3e12  # MI355X fp32 matrix (datasheet)
PEAK_BYTES = 8.0e12    # MI355X HBM3E (datasheet)


def torch_fp32(X):
    return X.sum(0), X.T @ X


def torch_fp64(X, rows=1 << 20):
    s = torch.zeros(X.shape[1], dtype=torch.float64, device=X.device)
    G = torch.zeros((X.shape[1], X.shape[1]), dtype=torch.float64, device=X.device)
    for i in range(0, X.shape[0], rows):
        Z = X[i:i + rows].double()
        s += Z.sum(0)
        G += Z.T @ Z
    return s, G


def validate(X, shift, rows=1 << 18):
    """moments on a sample against float64: ``(ok, worst error / bound)``."""
    xs = X[:rows].contiguous()
    slabs = Gm.default_slabs(len(xs), X.shape[1], X.device)
    s, G = Gm.moments(xs, shift=shift, slabs=slabs)
    zc = (xs - shift).double()
    f = Gm.error_factor(len(xs), slabs)
    a = zc.abs()
    share = max(float(((G - zc.T @ zc).abs() / (f * (a.T @ a))).max()), float(((s - zc.sum(0)).abs() / (f * a.sum(0))).max()))
    return bool(share <= 1) and bool(torch.equal(G, G.T)), share


def timed(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    out = fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b), out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=1 << 24)
    ap.add_argument("--steps", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--dims", default="16,64,128,256")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("bench_gram needs a GPU: nothing is measured without one")
    dev = torch.device("cuda", 0)
    box = torch.cuda.get_device_name(0)
    bad = 0
    for d in (int(v) for v in a.dims.split(",")):
        X = None
        g = torch.Generator(device=dev).manual_seed(1)
        X = torch.randn(a.n, d, device=dev, generator=g).add_(100.0)
        shift = X[:4096].double().mean(0).float()
        valid, share = validate(X, shift)
        fns = {"gram": lambda: Gm.moments(X, shift=shift), "torch_fp32": lambda: torch_fp32(X),
               "torch_fp64": lambda: torch_fp64(X)}
        times = {name: [] for name in fns}
        for fn in fns.values():
            for _ in range(a.warmup):
                fn()
        for _ in range(a.steps):  # alternate the partners, one timed call each per round
            for name, fn in fns.items():
                times[name].append(timed(fn)[0])
        ms = {name: statistics.median(t) for name, t in times.items()}
        read_ms = 4.0 * a.n * d / PEAK_BYTES * 1e3
        mfma_ms = 2.0 * a.n * d * d / 2 / PEAK_FLOPS * 1e3
        floor = max(read_ms, mfma_ms)
        row = {"box": box, "n": a.n, "d": d, "valid": valid, "worst_error_over_bound": round(share, 5),
               "slabs": Gm.default_slabs(a.n, d, dev), "gram_ms": round(ms["gram"], 3),
               "gram_ms_all": [round(t, 3) for t in times["gram"]], "torch_fp32_ms": round(ms["torch_fp32"], 3),
               "torch_fp64_ms": round(ms["torch_fp64"], 3), "fp32_over_gram": round(ms["torch_fp32"] / ms["gram"], 2),
               "fp64_over_gram": round(ms["torch_fp64"] / ms["gram"], 2), "read_floor_ms": round(read_ms, 3),
               "mfma_floor_ms": round(mfma_ms, 3), "bound_by": "read" if read_ms >= mfma_ms else "mfma",
               "floor_fraction": round(floor / ms["gram"], 3)}
        print(json.dumps(row), flush=True)
        bad += not valid
    sys.exit(1 if bad else 0)


if __name__ == "__main__":
    main()
