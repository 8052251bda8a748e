#!/usr/bin/env python
"""A/B of the segmented sort of ops/segments.py on one GPU: ``MR_SEG_SORT`` off
(one global radix sort by (list, value) and a gather) against on (the merge sort
of csrc/hip/segsort.hip), both in this process, alternating round by round.

Shapes: (a) ``latency`` — 4 M float64 values in 200 lists of 1/rank lengths
(nearly every value in a list of many tiles); (b) ``words`` — 4 M int64 values
in 300,000 lists of 1/rank lengths (nearly every list inside one tile); and
``examples/LatencyStats.device_reducefn`` on (a).  Every round times ``--iters``
calls between two device synchronisations; per variant the median, minimum and
maximum ms per call over the rounds are printed as one JSON line (the spread
of a variant is its max - min).  The two variants' outputs are compared bit
for bit at the timed sizes first.

    python tools/bench_segsort.py [--n 4000000] [--rounds 7] [--iters 50]
"""
from __future__ import annotations

import argparse
import dataclasses
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from lua_mapreduce_1_amd.examples import LatencyStats  # noqa: E402
from lua_mapreduce_1_amd.ops import segments as S  # noqa: E402


def knob(on: bool) -> None:
    S.TUNABLES = dataclasses.replace(S.TUNABLES, seg_sort=on)


def shape(n: int, m: int, dtype, dev):
    w = 1.0 / np.arange(1, m + 1)
    lens = np.floor(n * w / w.sum()).astype(np.int64)
    lens[0] += n - lens.sum()
    rng = np.random.default_rng(11)
    val = rng.lognormal(0.0, 0.7, n) if dtype == np.float64 else rng.integers(0, 1 << 40, n)
    off = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    return torch.from_numpy(off).to(dev), torch.from_numpy(val.astype(dtype)).to(dev)


def ms_per_call(fn, iters: int) -> float:
    torch.cuda.synchronize()
    t = time.perf_counter()
    for _ in range(iters):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t) * 1e3 / iters


def ab(name: str, fn, a) -> dict:
    outs = {}
    for on in (False, True):  # warm-up of both variants, and their results
        knob(on)
        for _ in range(3):
            outs[on] = fn()
    torch.cuda.synchronize()
    same = torch.equal(outs[False].view(torch.int64), outs[True].view(torch.int64))
    t = {False: [], True: []}
    for _ in range(a.rounds):
        for on in (False, True):
            knob(on)
            t[on].append(ms_per_call(fn, a.iters))
    r = {"case": name, "outputs_equal": same, "rounds": a.rounds, "iters": a.iters}
    for on, tag in ((False, "off"), (True, "on")):
        r[tag + "_ms"] = [round(x, 4) for x in t[on]]
        r[tag + "_median_ms"] = round(statistics.median(t[on]), 4)
        r[tag + "_spread_ms"] = round(max(t[on]) - min(t[on]), 4)
    return r


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=4_000_000)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--iters", type=int, default=50)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_segsort needs a GPU")
    dev = torch.device("cuda", 0)
    lat = shape(a.n, 200, np.float64, dev)
    words = shape(a.n, 300_000, np.int64, dev)
    bad = 0
    for name, fn in (("sort latency (200 lists, f64)", lambda: S.sort(*lat)),
                     ("sort words (300000 lists, i64)", lambda: S.sort(*words)),
                     ("LatencyStats.device_reducefn", lambda: LatencyStats.device_reducefn(None, *lat))):
        r = ab(name, fn, a)
        bad += not r["outputs_equal"]
        print(json.dumps(r), flush=True)
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
