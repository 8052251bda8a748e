#!/usr/bin/env python
"""A typed group-by (examples/ScoreStats: mean / max / count of a CSV column)
in the server + worker-processes shape under ``hbm`` storage, with
``MR_HBM_DEVICE_WRITE`` off and on in alternation: off is the host write side
(download, ``codec.encode_columns``, pinned upload), on has one encode launch
write the MRC2 map files into the worker's arena (csrc/hip/ipc.hip).

The corpus is tools/bench_generic.py's CSV shape (``corpus.score_csv``, seed
11, 300,000 words, 197 splits) as one file per split; every key of the final
answer is checked against the generator's own group-by.  One JSON line per
run (server time, ``Map sum(cpu_time)``, ``Reduce sum(cpu_time)`` of the
server's stats block) and one summary line.

``--job latency`` runs examples/LatencyStats instead (percentiles per endpoint
through ``device_reducefn``, no combiner: a list map whose MRL1 files hold
every value): with the knob on its map files are written by one encode launch
and its reduce jobs merge them on the device, with it off they are MRK1
records packed, merged and re-encoded on the host.  The log comes from the
example's ``make_log`` (seed 11), the answer is checked against its ``naive``.

    python tools/bench_hbm_cols.py [--job scores] [--lines 2000000] [--workers 1] [--repeat 3] [--storage hbm]
"""
from __future__ import annotations

import argparse
import json
import math
import os
import statistics
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

JOBS = {"scores": "lua_mapreduce_1_amd.examples.ScoreStats", "latency": "lua_mapreduce_1_amd.examples.LatencyStats"}


def serve(conn: str, db: str, storage: str, files: list[str], out: str, job: str = "scores") -> int:
    """The server process: one task of the job's module over ``files``; its stats
    block and the final answer go to ``out`` (msgpack)."""
    import importlib

    import msgpack
    from lua_mapreduce_1_amd import server
    from lua_mapreduce_1_amd.cli.execute_server import ensure_coordinator
    SS = JOBS[job]
    s = server.new(ensure_coordinator(conn), db)
    s.poll_sleep = 0.01
    s.quiet = True
    s.configure(dict(taskfn=SS, mapfn=SS, partitionfn=SS, reducefn=SS, finalfn=SS, init_args={"files": files},
                     storage=storage, device="auto"))
    time.sleep(2.0)  # (the workers connect)
    s.loop()
    with open(out, "wb") as f:
        f.write(msgpack.packb({"stats": s.last_stats, "result": importlib.import_module(SS).RESULT}))
    return 0


def run_once(a, rep: int, knob: bool, files: list[str], tmp: str) -> dict:
    conn, db = f"127.0.0.1:{a.port + rep}", f"cols{rep}"
    out = os.path.join(tmp, f"final.r{rep}.msgpack")
    env = dict(os.environ, PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", ""),
               MR_HBM_DEVICE_WRITE="1" if knob else "0")
    flist = os.path.join(tmp, "files.json")
    slog = open(os.path.join(tmp, f"server.r{rep}.txt"), "w")
    server = subprocess.Popen([sys.executable, os.path.abspath(__file__), "--serve", conn, db, a.storage, flist, out,
                               a.job],
                              stdout=subprocess.DEVNULL, stderr=slog, env=env)
    time.sleep(1.0)
    wlogs = [open(os.path.join(tmp, f"worker{i}.r{rep}.txt"), "w") for i in range(a.workers)]
    workers = [subprocess.Popen([sys.executable, os.path.join(ROOT, "execute_worker.py"), conn, db, "--poll", "0.01",
                                 "--max-iter", "1000", "--quiet"], stdout=subprocess.DEVNULL, stderr=wlogs[i], env=env)
               for i in range(a.workers)]
    try:
        server.wait(timeout=a.timeout)
    finally:
        if server.poll() is None:
            server.kill()
        for w in workers:
            w.terminate()
        for w in workers:
            try:
                w.wait(10)
            except subprocess.TimeoutExpired:
                w.kill()
        slog.close()
        for f in wlogs:
            f.close()
    r = {"rep": rep, "device_write": knob, "rc": server.returncode, "valid": False}
    if server.returncode == 0 and os.path.exists(out):
        import msgpack
        with open(out, "rb") as f:
            got = msgpack.unpackb(f.read(), strict_map_key=False)
        os.remove(out)
        st = got["stats"]
        r.update(server_time_s=st["iteration_time"], map_sum_cpu_time_s=st["map_sum_cpu_time"],
                 red_sum_cpu_time_s=st["red_sum_cpu_time"], failed_jobs=st["failed_map_jobs"] + st["failed_red_jobs"])
        r["result"] = got["result"]
    return r


def _close(a, b) -> bool:
    return len(a) == len(b) and all(math.isclose(x, y, rel_tol=1e-9, abs_tol=1e-9) for x, y in zip(a, b))


def main() -> int:
    if len(sys.argv) > 1 and sys.argv[1] == "--serve":
        conn, db, storage, flist, out = sys.argv[2:7]
        with open(flist) as f:
            return serve(conn, db, storage, json.load(f), out, *sys.argv[7:8])
    ap = argparse.ArgumentParser()
    ap.add_argument("--job", choices=sorted(JOBS), default="scores")
    ap.add_argument("--lines", type=int, default=2_000_000)
    ap.add_argument("--endpoints", type=int, default=5000, help="--job latency: distinct keys")
    ap.add_argument("--splits", type=int, default=64, help="--job latency: split files (map jobs)")
    ap.add_argument("--workers", type=int, default=1)
    ap.add_argument("--repeat", type=int, default=3, help="validated runs per setting (off, on, off, on, ...)")
    ap.add_argument("--storage", default="hbm")
    ap.add_argument("--port", type=int, default=27417)
    ap.add_argument("--timeout", type=float, default=300)
    a = ap.parse_args()
    from lua_mapreduce_1_amd.utils import corpus
    t0 = time.time()
    if a.job == "latency":
        import importlib
        ls = importlib.import_module(JOBS["latency"])
        splits = ls.make_log(seed=11, lines=a.lines, endpoints=a.endpoints, nsplits=a.splits)
        truth = ls.naive(splits)
    else:
        splits, truth = corpus.score_csv(seed=11, lines=a.lines, vocab_size=300_000,
                                         split_lines=max(1, a.lines // 197), return_truth=True)
    print(f"# generated {a.lines} CSV lines in {time.time() - t0:.1f}s", file=sys.stderr, flush=True)
    bad = 0
    runs = []
    with tempfile.TemporaryDirectory(prefix="lmr_hbm_cols_") as tmp:
        files = []
        for i, s in enumerate(splits):
            files.append(os.path.join(tmp, f"split{i:04d}.csv"))
            with open(files[-1], "wb") as f:
                f.write(s)
        with open(os.path.join(tmp, "files.json"), "w") as f:
            json.dump(files, f)
        del splits
        for rep in range(2 * a.repeat):
            r = run_once(a, rep, bool(rep % 2), files, tmp)
            got = r.pop("result", None)
            r["valid"] = (got is not None and r.get("failed_jobs") == 0 and got.keys() == truth.keys()
                          and all(_close(got[k], truth[k]) for k in truth))
            bad += not r["valid"]
            runs.append(r)
            print(json.dumps(r), flush=True)
    what = {"scores": "ScoreStats (CSV group-by: mean / max / count)",
            "latency": f"LatencyStats (p50 / p90 / p99 / max / count of {a.endpoints} endpoints, {a.splits} splits)"}
    out = {"job": what[a.job], "lines": a.lines, "workers": a.workers,
           "storage": a.storage, "valid_runs": len(runs) - bad, "runs": len(runs)}
    for knob in (False, True):
        ok = [r for r in runs if r["valid"] and r["device_write"] == knob]
        for k in ("server_time_s", "map_sum_cpu_time_s", "red_sum_cpu_time_s"):
            out[("on_" if knob else "off_") + k] = [round(r[k], 4) for r in ok]
            med = round(statistics.median(r[k] for r in ok), 4) if ok else None
            out[("on_" if knob else "off_") + k + "_median"] = med
    print(json.dumps(out), flush=True)
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
