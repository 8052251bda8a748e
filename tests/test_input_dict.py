"""Dictionary-coded input splits on the host (csrc/host/dictpack.cpp, ops/io.py
``dict_pack_splits``): every split decoded by a pure-Python decoder of the
format written here, the tile index checked against that decoder, the buffer
independent of the thread count, the form choice, and the MR_PACK_DICT knob of
the split store."""
import dataclasses

import numpy as np
import torch

from lua_mapreduce_1_amd.ops import io as mio
from lua_mapreduce_1_amd.parallel import splits as splitmod
from lua_mapreduce_1_amd.parallel.splits import SplitStore
from lua_mapreduce_1_amd.utils import corpus

LEAD = 0xC000
WS = b" \t\n\v\f\r"


def decode_units(units, slots):
    """(bytes, [(unit index, output offset) of every code]) of a unit stream."""
    out, starts, i = bytearray(), [], 0
    while i < len(units):
        u = int(units[i])
        starts.append((i, len(out)))
        if u < LEAD:
            e, i = u, i + 1
        else:
            assert i + 1 < len(units), "a lead is the last unit"
            v = int(units[i + 1])
            assert v < LEAD, "a lead is followed by a lead"
            e, i = LEAD + (u - LEAD) * LEAD + v, i + 2
        assert e < len(slots), "entry beyond the dictionary"
        ln = int(slots[e, 31])
        assert 1 <= ln <= 31
        out += bytes(slots[e, :ln])
    return bytes(out), starts


def pack(parts, threads=4, other=None, max_entries=mio.DICT_MAX_ENTRIES, force=False):
    parts = [np.frombuffer(bytes(p), dtype=np.uint8) for p in parts]
    off = np.concatenate([[0], np.cumsum([len(p) for p in parts])]).astype(np.int64)
    buf = torch.from_numpy(np.concatenate(parts + [np.zeros(0, dtype=np.uint8)]).copy())
    dk = mio.dict_pack_splits(buf, off, other_bytes=other, threads=threads, max_entries=max_entries, force=force)
    return dk, off, buf.numpy()


def check(parts, threads=4, max_entries=mio.DICT_MAX_ENTRIES):
    """Pack with every split forced into the dictionary form; decode and check
    every split and its tile index.  Returns the DictSplits."""
    dk, off, raw = pack(parts, threads, other=None, max_entries=max_entries)
    forced = pack(parts, threads, max_entries=max_entries, force=True)[0]
    slots = forced.slots
    assert np.array_equal(slots, dk.slots)
    assert 256 <= len(slots) <= max_entries
    for b in range(256):
        assert slots[b, 31] == 1 and slots[b, 0] == b and not slots[b, 1:31].any()
    assert len({bytes(s) for s in slots}) == len(slots)  # no entry twice
    codes = forced.buffer.numpy()
    for i in range(len(parts)):
        n = int(off[i + 1] - off[i])
        if n == 0:
            assert forced.nbytes[i] == 0
            continue
        assert forced.nbytes[i] == 2 * forced.units[i] > 0 and forced.offsets[i] % 16 == 0
        units = codes[int(forced.offsets[i]):int(forced.offsets[i] + forced.nbytes[i])].view("<u2")
        got, starts = decode_units(units, slots)
        assert got == bytes(raw[off[i]:off[i + 1]]), i
        r0, t = int(forced.trow[i]), int(forced.tiles[i])
        rows = forced.tix[r0:r0 + t + 1].astype(np.int64)
        assert t >= 1 and tuple(rows[0]) == (0, 0) and tuple(rows[-1]) == (len(units), n)
        code_at = dict(starts)
        for a, b in zip(rows[:-1], rows[1:]):
            assert int(a[0]) in code_at and code_at[int(a[0])] == int(a[1])  # a code boundary, at the right byte
            assert 1 <= b[0] - a[0] <= mio.DICT_TILE_UNITS and 1 <= b[1] - a[1] <= mio.DICT_TILE_BYTES
        # a split kept in the dictionary form by the real choice is coded the same
        if dk.nbytes[i]:
            assert np.array_equal(codes[int(forced.offsets[i]):int(forced.offsets[i] + forced.nbytes[i])],
                                  dk.buffer.numpy()[int(dk.offsets[i]):int(dk.offsets[i] + dk.nbytes[i])])
        assert dk.nbytes[i] in (0, forced.nbytes[i]) and (dk.nbytes[i] == 0) == (forced.nbytes[i] >= n)
    return forced


def words_text(rng, n, vocab=50):
    words = [bytes(rng.integers(97, 123, rng.integers(1, 9)).astype(np.uint8)) for _ in range(vocab)]
    out = bytearray()
    while len(out) < n:
        out += words[int(rng.integers(0, vocab))] + (b"\n" if rng.random() < 0.1 else b" ")
    return bytes(out[:n])


def test_round_trip_every_length():
    rng = np.random.default_rng(1)
    check([words_text(rng, n) for n in range(71)])


def test_round_trip_edges():
    rng = np.random.default_rng(2)
    nows = bytes(rng.integers(33, 127, 9000).astype(np.uint8))
    assert not any(c in WS for c in nows)
    t31, t32 = b"x" * 30 + b" ", b"y" * 31 + b" "
    parts = [corpus.tricky_text(rng, 20_000), nows, bytes(rng.choice(list(WS), 5000).astype(np.uint8)),
             bytes(range(256)) * 3, (t31 + t32) * 300, b"alpha beta alpha beta alpha", b"alpha beta " * 2000,
             words_text(rng, 70_001, vocab=400)]
    dk = check(parts)
    ents = {bytes(s[:s[31]]) for s in dk.slots[256:]}
    assert t31 in ents and t32 not in ents  # 31 bytes is the longest entry
    assert b"alpha " in ents and b"alpha" not in ents  # a last token without a separator is single bytes


def test_tiles_at_their_limits():
    """4096 single-byte codes per tile (no whitespace: nothing is a token), 31-byte
    entries up to 8192 output bytes per tile, and two-unit codes (more than
    48,896 entries) at tile and split ends."""
    rng = np.random.default_rng(3)
    nows = bytes(rng.integers(33, 127, 4096 * 2 + 5).astype(np.uint8))
    long31 = (b"z" * 30 + b"\n") * 600
    dk = check([nows, long31])
    t0 = dk.tix[int(dk.trow[0]):int(dk.trow[0] + dk.tiles[0] + 1)].astype(np.int64)
    assert (np.diff(t0[:, 0])[:2] == 4096).all()
    t1 = dk.tix[int(dk.trow[1]):int(dk.trow[1] + dk.tiles[1] + 1)].astype(np.int64)
    assert np.diff(t1[:, 1])[0] == 8192 // 31 * 31
    # a large vocabulary: the rare words get two-unit codes
    vocab = [b"w%05d " % i for i in range(60_000)]
    order = rng.permutation(60_000)
    # (50,000 words occur twice; the text ends with one that occurs once: those rank last)
    text = b"".join(vocab[i] for i in order[:50_000]) + b"".join(vocab[i] for i in order)
    dk = check([text, b"w00001 " * 3], threads=3)
    assert len(dk.slots) == 256 + 60_000
    units = dk.buffer.numpy()[int(dk.offsets[0]):int(dk.offsets[0] + dk.nbytes[0])].view("<u2")
    assert (units >= LEAD).any() and units[-2] >= LEAD  # the last code of the split is a two-unit code
    rows = dk.tix[int(dk.trow[0]):int(dk.trow[0] + dk.tiles[0] + 1), 0].astype(np.int64)
    assert any(units[r - 2] >= LEAD for r in rows[1:])  # ... and of some tile; none starts on a continuation
    assert not any(units[r - 1] >= LEAD for r in rows[1:])


def test_threads_do_not_change_the_result():
    rng = np.random.default_rng(4)
    parts = [words_text(rng, int(n), vocab=300) for n in rng.integers(0, 30_000, 23)] + [corpus.tricky_text(rng, 9000)]
    ref = None
    for threads in (1, 3, 16):
        dk, _, _ = pack(parts, threads)
        cur = (dk.slots.tobytes(), dk.nbytes.tobytes(), dk.offsets.tobytes(), dk.tix.tobytes())
        # (the 16-byte alignment gaps between splits are never written: compare the splits)
        body = [dk.buffer.numpy()[int(o):int(o + b)].tobytes() for o, b in zip(dk.offsets, dk.nbytes)]
        if ref is None:
            ref = (cur, body)
        assert (cur, body) == ref, threads


def test_entry_cap_and_form_choice():
    rng = np.random.default_rng(5)
    text = words_text(rng, 40_000, vocab=500)
    rand = bytes(rng.integers(0, 256, 5000).astype(np.uint8))
    ones = b"a" * 7 + b"\n"
    parts = [text, rand, ones * 400, b""]
    dk = check(parts, max_entries=300)
    assert len(dk.slots) == 300
    dk, off, _ = pack(parts)
    size = off[1:] - off[:-1]
    assert (dk.nbytes <= size).all() and dk.nbytes[0] > 0 and dk.nbytes[1] == 0 and dk.nbytes[3] == 0
    # against the k-bit form: the one-value split is 1 bit per byte there, smaller than its 2 bytes per token
    kbit = np.array([len(text) * 6 // 8, len(rand), 400, 0])
    dk, _, _ = pack(parts, other=kbit)
    assert dk.nbytes[0] > 0 and dk.nbytes[2] == 0 and (dk.nbytes <= kbit).all()
    assert dk.buffer.numel() == ((dk.nbytes + 15) // 16 * 16).sum()


def test_store_packs_once_and_knob(monkeypatch):
    parts = [b"aaaa", b"hello world\nhello world\nhello world foo bar", bytes(range(256)), b"x y z\n" * 40]
    on = dataclasses.replace(splitmod.TUNABLES, pack_input=True, pack_dict=True)
    off = dataclasses.replace(splitmod.TUNABLES, pack_input=True, pack_dict=False)
    assert type(on).from_env({"MR_PACK_DICT": "0"}).pack_dict is False
    assert type(on).from_env({"MR_PACK_DICT": "1"}).pack_dict is True
    monkeypatch.setattr(mio, "pinned_empty", lambda n: torch.empty(n, dtype=torch.uint8))

    def store(tun):
        monkeypatch.setattr(splitmod, "TUNABLES", tun)
        st = SplitStore(parts, pin=False)
        st._pinned = True  # a pinned store wants the packed copies (no GPU here: the memory itself is pageable)
        assert st.packed is None and st.dict_packed is None
        st.finish_loading()
        return st

    st = store(on)
    dk, pk = st.dict_packed, st.packed
    assert pk is not None and list(pk.k) == [1, 4, 8, 3]  # the k-bit copy is complete, as without the dictionary
    raw = st.buffer.numpy()
    size = np.diff(st.offsets)
    other = np.where(pk.k < 8, pk.nbytes, size)
    assert ((dk.nbytes == 0) | (dk.nbytes < other)).all() and dk.nbytes[1] > 0 and dk.nbytes[2] == 0
    for i in np.flatnonzero(dk.nbytes):
        a, b = st.region(int(i), int(i) + 1)
        units = dk.buffer.numpy()[int(dk.offsets[i]):int(dk.offsets[i] + dk.nbytes[i])].view("<u2")
        assert decode_units(units, dk.slots)[0] == bytes(raw[a:b])
    first = dk.buffer
    st.finish_loading()
    assert st.dict_packed.buffer is first and st.packed is pk  # packed once
    st0 = store(off)
    assert st0.dict_packed is None and st0.packed is not None
    pk0 = st0.packed  # (the alignment gaps between packed splits are never written: compare the splits)
    assert list(pk0.k) == list(pk.k) and list(pk0.offsets) == list(pk.offsets) and list(pk0.nbytes) == list(pk.nbytes)
    for o, b in zip(pk.offsets, pk.nbytes):
        assert np.array_equal(pk0.buffer.numpy()[int(o):int(o + b)], pk.buffer.numpy()[int(o):int(o + b)])
    plain = SplitStore(parts, pin=False)
    plain.finish_loading()
    assert plain.packed is None and plain.dict_packed is None
