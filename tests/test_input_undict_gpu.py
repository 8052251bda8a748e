"""Dictionary-coded input splits on the device: the decoder alone (csrc/hip/
undict.hip: alignments, length and tile edges, two-unit codes, bounded
behaviour on descriptors that do not fit) against the original bytes, and the
engine shipping all three forms (parallel/staging.py) against the same engine
shipping raw bytes."""
import numpy as np
import pytest
import torch

from lua_mapreduce_1_amd.ops import io as mio
from lua_mapreduce_1_amd.utils import corpus

pytestmark = pytest.mark.gpu

SENTINEL = 0xEE
GUARD = 64
LEAD = 0xC000
M = "lua_mapreduce_1_amd.models.wordcount"


def _words(rng, n, vocab=60):
    words = [bytes(rng.integers(97, 123, rng.integers(1, 9)).astype(np.uint8)) for _ in range(vocab)]
    out = bytearray()
    while len(out) < n:
        out += words[int(rng.integers(0, vocab))] + (b"\n" if rng.random() < 0.1 else b" ")
    return bytes(out[:n])


def _pack(parts):
    arrs = [np.frombuffer(p, dtype=np.uint8) for p in parts]
    off = np.concatenate([[0], np.cumsum([len(p) for p in arrs])]).astype(np.int64)
    raw = np.concatenate(arrs)
    assert SENTINEL not in raw
    return mio.dict_pack_splits(torch.from_numpy(raw.copy()), off, threads=4, force=True), off, raw


def _decode(dk, off, start, nb, sel=None, entries=None, tix=None, size=None):
    """One launch over the splits ``sel`` (default: all) into a sentinel-filled
    arena of ``nb`` bytes, split i at ``start + off[i]``; returns the arena."""
    from lua_mapreduce_1_amd.ops import _hip
    dev = torch.device("cuda", 0)
    sel = np.arange(len(off) - 1) if sel is None else np.asarray(sel)
    size = (off[1:] - off[:-1]) if size is None else np.asarray(size, dtype=np.int64)
    desc = np.zeros((len(sel), 4), dtype=np.int64)
    desc[:, 0] = dk.offsets[sel]
    desc[:, 1] = start + off[:-1][sel]
    desc[:, 2] = size[sel] | (dk.units[sel] << 32)
    desc[:, 3] = dk.trow[sel] | (dk.tiles[sel] << 32)
    arena = torch.full((nb,), SENTINEL, dtype=torch.uint8, device=dev)
    codes = dk.buffer.to(dev)
    d_desc = torch.from_numpy(desc).to(dev)
    d_tix = torch.from_numpy((dk.tix if tix is None else tix).view(np.int32)).to(dev)
    d_slots = torch.from_numpy(dk.slots).to(dev)
    _hip.call("mr_undict_splits", _hip.ptr(codes), codes.numel(), _hip.ptr(arena), arena.numel(), _hip.ptr(d_desc),
              len(sel), int(dk.tiles[sel].max()), _hip.ptr(d_tix), d_tix.shape[0], _hip.ptr(d_slots),
              len(dk.slots) if entries is None else entries, _hip.stream(dev))
    torch.cuda.synchronize()
    return arena.cpu().numpy()


@pytest.fixture(scope="module")
def edge_splits():
    """Splits of 1, 15, 16, 17 and 8193 bytes, 4096 single-byte codes in a tile
    (no whitespace: nothing is a token), a tile of exactly 8192 output bytes
    made of 31-byte entries, and word text over several tiles."""
    rng = np.random.default_rng(21)
    nows = bytes(rng.integers(33, 127, 2 * 4096 + 5).astype(np.uint8))
    full = (b"z" * 30 + b"\n") * 264 + b"abcdefg\n" + (b"z" * 30 + b"\n") * 40
    parts = [_words(rng, n) for n in (1, 15, 16, 17, 8193)] + [nows, b"q", full, _words(rng, 30_011, vocab=300),
                                                                 _words(rng, 2, vocab=3), _words(rng, 70_001, vocab=2000)]
    dk, off, raw = _pack(parts)
    rows = lambda i: dk.tix[int(dk.trow[i]):int(dk.trow[i] + dk.tiles[i] + 1)].astype(np.int64)  # noqa: E731
    assert (np.diff(rows(5)[:, 0])[:2] == 4096).all()  # 4096 single-byte codes
    assert np.diff(rows(7)[:, 1])[0] == 8192 and len({int(t) for t in dk.tiles}) >= 4
    return dk, off, raw


def test_decoder_alone_every_alignment(edge_splits):
    """Every split exact, every other byte (64 guard bytes in front and behind)
    untouched: all splits in two layouts, and the splits of 1, 15, 16, 17, 8193
    and 2 bytes at each of the 16 destination alignments."""
    dk, off, raw = edge_splits
    small = [0, 1, 2, 3, 4, 6, 9]
    for start in range(GUARD, GUARD + 16):
        nb = start + int(off[-1]) + GUARD
        got = _decode(dk, off, start, nb, sel=small)
        want = np.full(nb, SENTINEL, dtype=np.uint8)
        for i in small:
            want[start + off[i]:start + off[i + 1]] = raw[off[i]:off[i + 1]]
        assert np.array_equal(got, want), start
    for start in (GUARD, GUARD + 5):
        nb = start + int(off[-1]) + GUARD
        got = _decode(dk, off, start, nb)
        want = np.full(nb, SENTINEL, dtype=np.uint8)
        want[start:start + int(off[-1])] = raw
        for i in range(len(off) - 1):
            assert np.array_equal(got[start + off[i]:start + off[i + 1]], raw[off[i]:off[i + 1]]), (start, i)
        assert np.array_equal(got, want)
    # a launch over some of the splits leaves the others' bytes alone
    sel = [1, 4, 7, 9]
    got = _decode(dk, off, GUARD, nb, sel=sel)
    want = np.full(nb, SENTINEL, dtype=np.uint8)
    for i in sel:
        want[GUARD + off[i]:GUARD + off[i + 1]] = raw[off[i]:off[i + 1]]
    assert np.array_equal(got, want)


@pytest.fixture(scope="module")
def big_vocab():
    """60,000 distinct words: the rare ones get two-unit codes; the split ends
    with one, and so does some tile."""
    rng = np.random.default_rng(22)
    vocab = [b"w%05d " % i for i in range(60_000)]
    order = rng.permutation(60_000)
    text = b"".join(vocab[i] for i in order[:50_000]) + b"".join(vocab[i] for i in order)
    dk, off, raw = _pack([b"w00001 w00002 ", text])
    units = dk.buffer.numpy()[int(dk.offsets[1]):int(dk.offsets[1] + dk.nbytes[1])].view("<u2")
    rows = dk.tix[int(dk.trow[1]):int(dk.trow[1] + dk.tiles[1] + 1), 0].astype(np.int64)
    assert units[-2] >= LEAD and any(units[r - 2] >= LEAD for r in rows[1:-1])
    return dk, off, raw, units, rows


def test_two_unit_codes_at_tile_and_split_ends(big_vocab):
    dk, off, raw, _, _ = big_vocab
    nb = GUARD + 3 + int(off[-1]) + GUARD
    got = _decode(dk, off, GUARD + 3, nb)
    want = np.full(nb, SENTINEL, dtype=np.uint8)
    want[GUARD + 3:GUARD + 3 + int(off[-1])] = raw
    assert np.array_equal(got, want)


def test_descriptors_that_do_not_fit_write_nothing_outside(big_vocab, edge_splits):
    """Bounded inputs: a dictionary shorter than the entries the stream names, a
    split whose descriptor is shorter than its tile index says, and a tile
    index cut behind a lead.  Nothing outside the splits' ranges is written
    (guards and the neighbouring split stay), and what fits is still exact."""
    dk, off, raw, units, rows = big_vocab
    start = GUARD + 7
    nb = start + int(off[-1]) + GUARD
    want = np.full(nb, SENTINEL, dtype=np.uint8)
    want[start:start + int(off[-1])] = raw
    # entries beyond the dictionary: those codes write nothing (their bytes keep what the LDS image held)
    got = _decode(dk, off, start, nb, entries=LEAD)
    assert np.array_equal(got[:start + off[1]], want[:start + off[1]])  # front guard and the first split
    assert np.array_equal(got[start + off[2]:], want[start + off[2]:])  # back guard
    # the second split's range is one byte short of what its index says: its last tile is skipped whole
    size = (off[1:] - off[:-1]).copy()
    size[1] -= 1
    got = _decode(dk, off, start, nb, size=size)
    last = int(dk.tix[int(dk.trow[1] + dk.tiles[1] - 1), 1])
    assert np.array_equal(got[:start + off[1] + last], want[:start + off[1] + last])
    assert (got[start + off[1] + last:] == SENTINEL).all()
    # a tile boundary moved behind a lead: the tile in front ends on the lead, the next starts on its continuation
    t = next(int(j) for j in range(1, len(rows) - 1) if units[rows[j] - 2] >= LEAD)
    tix = dk.tix.copy()
    tix[int(dk.trow[1]) + t, 0] -= 1
    tix[int(dk.trow[1]) + t, 1] -= 7  # (the two-unit code in front decodes to 7 bytes)
    got = _decode(dk, off, start, nb, tix=tix)
    assert np.array_equal(got[:start + off[1]], want[:start + off[1]])
    assert np.array_equal(got[start + off[2]:], want[start + off[2]:])
    lo, hi = int(tix[int(dk.trow[1]) + t - 1, 1]), int(dk.tix[int(dk.trow[1]) + t + 1, 1])
    inner = np.ones(int(off[2] - off[1]), dtype=bool)
    inner[lo:hi] = False  # (the two tiles around the moved boundary)
    assert np.array_equal(got[start + off[1]:start + off[2]][inner], raw[off[1]:off[2]][inner])
    # a descriptor past the arena's end is skipped
    dk2, off2, raw2 = edge_splits
    got = _decode(dk2, off2, GUARD, GUARD + int(off2[-1]) - 1)
    assert np.array_equal(got[GUARD:GUARD + off2[-2]], raw2[:off2[-2]]) and (got[GUARD + off2[-2]:] == SENTINEL).all()


@pytest.fixture(scope="module")
def small_store():
    from lua_mapreduce_1_amd.parallel.spmd import SplitStore
    rng = np.random.default_rng(7)  # (174 distinct byte values in 6000 bytes: the split stays raw)
    parts = [(b"a" * 7 + b"\n") * 400, corpus.tricky_text(rng, 6000)]
    parts += corpus.europarl_like(seed=3, lines=600, words=9000, split_lines=100)[:4]
    assert len(parts) == 6
    store = SplitStore(parts, pin=True)
    store.finish_loading(pack=True, pack_dict=True)
    pk, dk = store.packed, store.dict_packed
    assert pk.k[0] == 1 and pk.k[1] == 8 and (pk.k[2:] < 8).all()  # the k-bit copy is what it was
    assert list(dk.nbytes > 0) == [False, False, True, True, True, True]
    return store


def _engine(store, pack: bool, pack_dict: bool = True):
    from lua_mapreduce_1_amd.parallel.spmd import SPMDEngine
    # chunks of a few KB: several chunks per plan, the first with a split of each form
    return SPMDEngine(dict(taskfn=M, mapfn=M, partitionfn=M, reducefn=M, finalfn=M, pack_input=pack,
                           pack_dict=pack_dict, init_args={"nsplits": len(store), "num_reducers": 3}),
                      split_store=store, device=torch.device("cuda", 0), chunk_mb=(0.009, 0.012), tail_mb=(0.006,))


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
    assert not eng._ships_packed() and not eng._ships_dict()
    res = eng.run_iteration(prefetch_next=False)
    out = _parts(res)
    assert all(p[5] is None for p in eng._plans.values()) and not any(eng._pack_staging)
    return out


def test_engine_three_forms_match_raw(small_store, raw_result):
    """3 iterations with prefetch: the chunked plan and the prefetched
    single-copy plan both decode into arenas byte-identical to the host buffer,
    every iteration's partitions equal the raw engine's, and one chunk holds a
    dictionary-coded, a k-bit and a raw split."""
    eng = _engine(small_store, True)
    assert eng._ships_dict()
    eng.prefetch = True
    for q in range(3):
        res = eng.run_iteration(prefetch_next=q < 2, lookahead=2 - q)
        _same(_parts(res), raw_result)
        _arena_ok(eng, small_store, q)
    kinds = {(k[3], p[5] is not None and "dict" in p[5]) for k, p in eng._plans.items()}
    assert (False, True) in kinds and all(coded for _, coded in kinds)
    chunked = next(p for k, p in eng._plans.items() if not k[3])
    assert len(chunked[0]) > 2 and any(c["raw"] and c["nd"] and c["dnd"] for c in chunked[5]["chunks"])
    for c in chunked[5]["chunks"]:  # per chunk only its own code units and k-bit bytes cross the link
        assert c["ddev"].numel() == c["dhost"].numel() and c["dev"].numel() == c["host"].numel()
    st = small_store
    shipped = sum(c["ddev"].numel() for c in chunked[5]["chunks"])  # (the units, and alignment gaps inside a chunk)
    assert int(st.dict_packed.nbytes.sum()) <= shipped <= int(((st.dict_packed.nbytes + 15) // 16 * 16).sum())
    assert sum(c["dev"].numel() for c in chunked[5]["chunks"]) == int(st.packed.nbytes[0])


def test_engine_three_forms_resident(small_store, raw_result):
    """resident=True: the arena filled through the decoders is mapped in place
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


def test_engine_knob_off_is_the_packed_plan(small_store, raw_result):
    """pack_dict=False on a store that holds the dictionary copy: the plan of
    the k-bit engine, nothing of the dictionary form in it."""
    eng = _engine(small_store, True, pack_dict=False)
    assert eng._ships_packed() and not eng._ships_dict()
    res = eng.run_iteration(prefetch_next=False)
    _same(_parts(res), raw_result)
    _arena_ok(eng, small_store, 0)
    assert all(p[5] is not None and "dict" not in p[5] and all("ddev" not in c for c in p[5]["chunks"])
               for p in eng._plans.values())
    assert all(k[4] is True for k in eng._plans) and eng._dict_dev is None
