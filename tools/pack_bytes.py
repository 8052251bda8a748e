"""Raw, bit-packed and dictionary-coded size of the benchmark corpus: the
histogram of the code widths of its splits (csrc/host/pack.cpp), and the
dictionary form's bytes, entries, dictionary size and pack time (csrc/host/
dictpack.cpp); CPU only.

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
    store.finish_loading(pack=True, pack_dict=False)
    dt = time.perf_counter() - t0
    t0 = time.perf_counter()
    store.finish_loading(pack=True, pack_dict=True)
    ddt = time.perf_counter() - t0
    dk = store.dict_packed
    pk = store.packed
    raw = int(store.buffer.numel())
    hist = collections.Counter(int(k) for k in pk.k)
    odd = [i for i, k in enumerate(pk.k) if k != 6]
    print(json.dumps({"splits": len(store), "raw_bytes": raw, "packed_bytes": int(pk.buffer.numel()),
                      "ratio": pk.buffer.numel() / raw, "width_histogram": dict(sorted(hist.items())),
                      "splits_not_6_bits": odd, "pack_seconds": dt, "threads": args.threads,
                      "dict_bytes": int(dk.buffer.numel()), "dict_ratio": dk.buffer.numel() / raw,
                      "dict_splits": int((dk.nbytes > 0).sum()), "dict_entries": int(len(dk.slots)),
                      "dict_one_unit_entries": int(min(len(dk.slots), 0xC000)),
                      "dictionary_bytes": int(dk.slots.nbytes), "tile_index_bytes": int(dk.tix.nbytes),
                      "dict_pack_seconds": ddt, "dict_threads": max(args.threads, 16)}))
    return 0


if __name__ == "__main__":
    sys.exit(main())
