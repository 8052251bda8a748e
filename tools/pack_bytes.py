"""Raw and bit-packed size of the benchmark corpus and the histogram of the
code widths of its splits (csrc/host/pack.cpp); CPU only.

    python tools/pack_bytes.py [--threads 8]
"""
import argparse
import collections
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--threads", type=int, default=8)
    args = ap.parse_args()
    import bench
    from lua_mapreduce_1_amd.parallel.splits import SplitStore
    from lua_mapreduce_1_amd.utils import corpus
    d = bench.corpus_dir(1234, corpus.EUROPARL_LINES, corpus.EUROPARL_WORDS)
    bench.ensure_corpus(d, 1234, corpus.EUROPARL_LINES, corpus.EUROPARL_WORDS)
    store = SplitStore.from_blob(os.path.join(d, "blob.bin"), np.load(os.path.join(d, "off.npy")), pin=False,
                                 threads=args.threads)
    store.finish_loading(pack=False)
    t0 = time.perf_counter()
    store.finish_loading(pack=True)
    dt = time.perf_counter() - t0
    pk = store.packed
    raw = int(store.buffer.numel())
    hist = collections.Counter(int(k) for k in pk.k)
    odd = [i for i, k in enumerate(pk.k) if k != 6]
    print(json.dumps({"splits": len(store), "raw_bytes": raw, "packed_bytes": int(pk.buffer.numel()),
                      "ratio": pk.buffer.numel() / raw, "width_histogram": dict(sorted(hist.items())),
                      "splits_not_6_bits": odd, "pack_seconds": dt, "threads": args.threads}))
    return 0


if __name__ == "__main__":
    sys.exit(main())
