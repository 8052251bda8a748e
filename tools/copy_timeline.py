"""Copy-stream timeline of the headline run from device events: every
host -> HBM copy of the timed steps is bracketed by two timing events on the
copy stream (no profiler), giving the bytes shipped per step, the achieved
H2D rate, the copy engine's busy time per step and the gaps between
consecutive copies.  The brackets cost a little host time per copy, so the
step time printed here is not the headline's.

    python tools/copy_timeline.py [--steps 20 --warmup 5]      (MR_PACK_INPUT=0|1, MR_PACK_DICT=0|1)
"""
import argparse
import gc
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    args = ap.parse_args()
    import bench
    from lua_mapreduce_1_amd.ops import _hip
    from lua_mapreduce_1_amd.parallel.spmd import SPMDEngine, SplitStore
    from lua_mapreduce_1_amd.utils import corpus
    from lua_mapreduce_1_amd.utils.config import TUNABLES
    device = torch.device("cuda", 0)
    torch.zeros(1, device=device)
    d = bench.corpus_dir(1234, corpus.EUROPARL_LINES, corpus.EUROPARL_WORDS)
    bench.ensure_corpus(d, 1234, corpus.EUROPARL_LINES, corpus.EUROPARL_WORDS)
    store = SplitStore.from_blob(os.path.join(d, "blob.bin"), np.load(os.path.join(d, "off.npy")))
    store.finish_loading()
    M = bench.MODEL
    eng = SPMDEngine(dict(taskfn=M, mapfn=M, partitionfn=M, reducefn=M, finalfn=M,
                          init_args={"nsplits": len(store), "num_reducers": 10}), device=device, split_store=store)
    eng.prefetch, eng.pipeline = True, TUNABLES.pipeline
    gc.collect()
    gc.freeze()
    for w in range(args.warmup):
        eng.run_iteration(prefetch_next=w < args.warmup - 1, lookahead=args.warmup - 1 - w)
    torch.cuda.synchronize(device)

    log = []  # (event before, event after, bytes) of every H2D copy on the copy stream
    real = _hip.call
    cs_ptr = eng.copy_stream.cuda_stream

    def call(name, *a):
        if name == "mr_memcpy_async" and a[3] == 1 and a[4].value == cs_ptr:
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(eng.copy_stream)
            real(name, *a)
            e1.record(eng.copy_stream)
            log.append((e0, e1, int(a[2])))
        else:
            real(name, *a)

    _hip.call = call
    t0 = time.perf_counter()
    last = None
    for i in range(args.steps):
        last = eng.run_iteration(prefetch_next=i < args.steps - 1, lookahead=args.steps - 1 - i)
    last.wait()
    torch.cuda.synchronize(device)
    ms = 1000.0 * (time.perf_counter() - t0) / args.steps
    _hip.call = real
    base = log[0][0]
    spans = [(base.elapsed_time(a), base.elapsed_time(b), n) for a, b, n in log]
    busy = sum(b - a for a, b, _ in spans)
    nbytes = sum(n for _, _, n in spans)
    gaps = [spans[i + 1][0] - spans[i][1] for i in range(len(spans) - 1)]
    big = [(b - a, n) for a, b, n in spans if n >= 32 << 20]
    print(json.dumps({
        "pack_input": eng._ships_packed(), "pack_dict": eng._ships_dict(), "steps": args.steps, "ms_per_step_with_brackets": ms,
        "copies": len(spans), "h2d_bytes_per_step": nbytes / args.steps, "copy_busy_ms_per_step": busy / args.steps,
        "h2d_GBps_copies_of_32MiB_up": sum(n for _, n in big) / max(sum(t for t, _ in big), 1e-9) / 1e6,
        "first_copy_to_last_copy_end_ms": spans[-1][1] - spans[0][0],
        "gap_ms_total_per_step": sum(gaps) / args.steps, "gap_ms_max": max(gaps) if gaps else 0.0,
        "gaps_ms": [round(g, 3) for g in gaps]}))
    return 0


if __name__ == "__main__":
    sys.exit(main())
