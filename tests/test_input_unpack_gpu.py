"""Bit-packed input splits on the device: the unpack kernel alone (csrc/hip/
unpack.hip: every width, the length and alignment edges, neighbours untouched)
and the engine shipping the packed store (parallel/staging.py) against the
same engine shipping raw bytes."""
import numpy as np
import pytest
import torch

from lua_mapreduce_1_amd.ops import io as mio
from lua_mapreduce_1_amd.utils import corpus

pytestmark = pytest.mark.gpu

SENTINEL = 0xEE
GUARD = 64
M = "lua_mapreduce_1_amd.models.wordcount"


def _split(rng, alphabet: int, n: int) -> np.ndarray:
    vals = rng.permutation(256)[:alphabet].astype(np.uint8)
    vals = vals[vals != SENTINEL] if alphabet > 1 else np.array([0x41], dtype=np.uint8)
    s = vals[rng.integers(0, len(vals), n)]
    m = min(len(vals), n)
    s[rng.permutation(n)[:m]] = vals[:m]
    return s


def test_unpack_kernel_alone():
    """One launch over 14 splits of widths 1..7 and lengths 1, 15, 16, 17, 63,
    64, 65, 4097 and 70,001, back to back in an arena pre-filled with a
    sentinel (no split holds that byte), every destination residue mod 16
    present: every split exact, every other byte — the 64 guard bytes in front
    and behind included — untouched."""
    from lua_mapreduce_1_amd.ops import _hip
    dev = torch.device("cuda", 0)
    rng = np.random.default_rng(11)
    # (alphabet, length): widths 1..7; the 1-byte lengths walk the residues
    shapes = [(2, 1), (3, 15), (5, 16), (2, 17), (9, 63), (17, 64), (33, 65), (65, 4097), (59, 70_001), (128, 1),
              (4, 1), (1, 65), (100, 4097), (60, 17)]
    splits = [_split(rng, a, n) for a, n in shapes]
    off = np.concatenate([[0], np.cumsum([len(s) for s in splits])]).astype(np.int64)
    pk = mio.pack_splits(torch.from_numpy(np.concatenate(splits)), off, threads=4)
    assert set(int(k) for k in pk.k) == {1, 2, 3, 4, 5, 6, 7}
    starts = (GUARD, GUARD + 8)  # two layouts: all 16 residues of the destination occur
    assert {int(d) % 16 for st in starts for d in st + off[:-1]} == set(range(16))
    for start in starts:
        dst = start + off[:-1]
        nb = start + int(off[-1]) + GUARD
        arena = torch.full((nb,), SENTINEL, dtype=torch.uint8, device=dev)
        staging = pk.buffer.to(dev)
        desc = np.zeros((len(splits), 4), dtype=np.int64)
        desc[:, 0], desc[:, 1], desc[:, 2] = pk.offsets, dst, off[1:] - off[:-1]
        desc[:, 3] = pk.k.astype(np.int64) | ((np.arange(len(splits), dtype=np.int64) * 128) << 32)
        d_desc = torch.from_numpy(desc).to(dev)
        d_tab = torch.from_numpy(np.ascontiguousarray(pk.tables).reshape(-1)).to(dev)
        _hip.call("mr_unpack_splits", _hip.ptr(staging), staging.numel(), _hip.ptr(arena), arena.numel(),
                  _hip.ptr(d_desc), len(splits), int(desc[:, 2].max()), _hip.ptr(d_tab), d_tab.numel(),
                  _hip.stream(dev))
        got = arena.cpu().numpy()
        want = np.full(nb, SENTINEL, dtype=np.uint8)
        want[start:start + int(off[-1])] = np.concatenate(splits)
        for i, s in enumerate(splits):
            assert np.array_equal(got[dst[i]:dst[i] + len(s)], s), (start, i, shapes[i])
        assert np.array_equal(got, want)


@pytest.fixture(scope="module")
def small_store():
    from lua_mapreduce_1_amd.parallel.spmd import SplitStore
    rng = np.random.default_rng(7)  # (174 distinct byte values in 6000 bytes: the split stays raw)
    parts = [(b"a" * 7 + b"\n") * 400, corpus.tricky_text(rng, 6000)]
    parts += corpus.europarl_like(seed=3, lines=600, words=9000, split_lines=100)[:4]
    assert len(parts) == 6
    store = SplitStore(parts, pin=True)
    store.finish_loading(pack=True)
    assert store.packed is not None and store.packed.k[0] == 1 and store.packed.k[1] == 8
    assert (store.packed.k[2:] < 8).all()
    return store


def _engine(store, pack: bool):
    from lua_mapreduce_1_amd.parallel.spmd import SPMDEngine
    # chunks of a few KB: several chunks per plan, the raw split inside one
    return SPMDEngine(dict(taskfn=M, mapfn=M, partitionfn=M, reducefn=M, finalfn=M, pack_input=pack,
                           init_args={"nsplits": len(store), "num_reducers": 3}),
                      split_store=store, device=torch.device("cuda", 0), chunk_mb=(0.004, 0.012), tail_mb=(0.006,))


def _parts(res):
    return {p: {k: (None if v is None else np.array(v)) for k, v in cols.items()} for p, cols in
            res.partitions.items()}


def _same(a, b):
    assert a.keys() == b.keys()
    for p in a:
        assert a[p].keys() == b[p].keys()
        for k in a[p]:
            assert (a[p][k] is None) == (b[p][k] is None), (p, k)
            if a[p][k] is not None:
                assert np.array_equal(a[p][k], b[p][k]), (p, k)


def _arena_ok(eng, store, q):
    torch.cuda.synchronize()
    arena = eng.arenas[q % 3]
    n = store.buffer.numel()
    assert torch.equal(arena[:n].cpu(), store.buffer)


@pytest.fixture(scope="module")
def raw_result(small_store):
    eng = _engine(small_store, False)
    assert not eng._ships_packed()
    res = eng.run_iteration(prefetch_next=False)
    out = _parts(res)
    assert all(p[5] is None for p in eng._plans.values()) and not any(eng._pack_staging)
    return out


def test_engine_packed_matches_raw(small_store, raw_result):
    """3 iterations with prefetch: the chunked plan (first iteration) and the
    prefetched single-copy plan both unpack into arenas byte-identical to the
    host buffer, and every iteration's partitions equal the raw engine's."""
    eng = _engine(small_store, True)
    assert eng._ships_packed()
    eng.prefetch = True
    for q in range(3):
        res = eng.run_iteration(prefetch_next=q < 2, lookahead=2 - q)
        _same(_parts(res), raw_result)
        _arena_ok(eng, small_store, q)
    kinds = {(k[3], p[5] is not None) for k, p in eng._plans.items()}
    assert (False, True) in kinds and all(packed for _, packed in kinds)
    chunked = next(p for k, p in eng._plans.items() if not k[3])
    assert len(chunked[0]) > 2 and any(c["raw"] for c in chunked[5]["chunks"])


def test_engine_packed_resident(small_store, raw_result):
    """resident=True: the arena filled through the unpack is mapped in place
    by the later iterations."""
    eng = _engine(small_store, True)
    eng.prefetch = True
    eng.resident = True
    for q in range(4):
        res = eng.run_iteration(prefetch_next=q < 3, lookahead=3 - q)
        _same(_parts(res), raw_result)
    for q in range(3):
        if eng._arena_holds.get(q) is not None:
            _arena_ok(eng, small_store, q)
