"""The host packer of the input splits (csrc/host/pack.cpp through
libmrhost.so) against a numpy decoder written here: exact round trips, minimum
widths, aligned offsets and exact sizes over the alphabet sizes and split
lengths at which the packer takes another path; and the MR_PACK_INPUT knob of
the split store."""
import dataclasses

import numpy as np
import pytest
import torch

from lua_mapreduce_1_amd.ops import io as mio
from lua_mapreduce_1_amd.parallel import splits as splitmod
from lua_mapreduce_1_amd.parallel.splits import SplitStore
from lua_mapreduce_1_amd.utils import corpus

ALPHABETS = [1, 2, 3, 16, 17, 59, 64, 65, 128, 129, 256]
LENGTHS = [1, 15, 16, 17, 31, 33, 4095, 4096, 4097, 70_001]


def decode(packed: np.ndarray, k: int, n: int, table: np.ndarray) -> np.ndarray:
    """Bytes of one packed split: groups of 16 k-bit codes, 2k bytes each,
    symbol i of a group in bits [k i, k i + k) of the group as a little-endian
    integer; code -> byte through ``table``."""
    groups = (n + 15) // 16
    bits = np.unpackbits(packed[:groups * 2 * k], bitorder="little").reshape(groups * 16, k)
    codes = (bits.astype(np.int64) << np.arange(k)).sum(axis=1)
    assert not codes[n:].any(), "the last group is zero-padded"
    return table[codes[:n]]


def min_width(distinct: int) -> int:
    if distinct > 128:
        return 8
    k = 1
    while (1 << k) < distinct:
        k += 1
    return k


def make_split(rng, alphabet: int, n: int) -> np.ndarray:
    """n bytes over `alphabet` random byte values; min(alphabet, n) of them occur."""
    vals = rng.permutation(256)[:alphabet].astype(np.uint8)
    s = vals[rng.integers(0, alphabet, n)]
    m = min(alphabet, n)
    s[rng.permutation(n)[:m]] = vals[:m]
    return s


def check(splits: list[np.ndarray], threads: int = 4) -> mio.PackedSplits:
    buf = torch.from_numpy(np.concatenate(splits))
    off = np.concatenate([[0], np.cumsum([len(s) for s in splits])]).astype(np.int64)
    pk = mio.pack_splits(buf, off, threads=threads)
    at = 0
    for i, s in enumerate(splits):
        k = min_width(len(np.unique(s)))
        assert pk.k[i] == k, (i, pk.k[i], k)
        assert pk.offsets[i] % 16 == 0 and pk.offsets[i] == at
        if k == 8:  # raw: no packed bytes, no table
            assert pk.nbytes[i] == 0 and not pk.tables[i].any()
            continue
        assert pk.nbytes[i] == (len(s) + 15) // 16 * 2 * k
        at += (int(pk.nbytes[i]) + 15) // 16 * 16
        a = len(np.unique(s))
        assert (np.diff(pk.tables[i][:a].astype(int)) > 0).all() and not pk.tables[i][a:].any()
        got = decode(pk.buffer.numpy()[int(pk.offsets[i]):int(pk.offsets[i] + pk.nbytes[i])], k, len(s), pk.tables[i])
        assert np.array_equal(got, s), i
    assert pk.buffer.numel() == at
    return pk


@pytest.mark.parametrize("alphabet", ALPHABETS)
def test_round_trip_every_length(alphabet):
    """One store per alphabet size, a split of every length: exact round
    trip, minimum k (129 and 256 values come back raw), 16-aligned offsets,
    ceil(n / 16) * 2k packed bytes."""
    rng = np.random.default_rng(1000 + alphabet)
    pk = check([make_split(rng, alphabet, n) for n in LENGTHS])
    if alphabet > 128:
        assert (pk.k[[n >= alphabet for n in LENGTHS]] == 8).all()


def test_tricky_text_and_mixed_widths():
    """Adversarial text (NULs, high bytes), and one store whose splits have
    different widths, packed by more threads than splits and by one."""
    rng = np.random.default_rng(7)
    tricky = np.frombuffer(corpus.tricky_text(rng, 40_000), dtype=np.uint8).copy()
    mixed = [make_split(rng, a, n) for a, n in ((1, 100), (2, 33), (5, 4097), (59, 70_001), (100, 999), (200, 5000),
                                                (9, 16), (33, 17))]
    for threads in (1, 32):
        pk = check([tricky] + mixed + [np.zeros(40, dtype=np.uint8)], threads=threads)
        assert list(pk.k[1:]) == [1, 1, 3, 6, 7, 8, 4, 5, 1]  # (33 values, 17 bytes: 17 occur)
        assert pk.k[0] == min_width(len(np.unique(tricky)))


def test_store_packs_when_loading_finishes(tmp_path, monkeypatch):
    """finish_loading() packs a store that wants it (the padding newline is
    part of the split), keeps the raw buffer, and with MR_PACK_INPUT=0 the store
    has no packed buffer."""
    parts = [b"aaaa", b"hello world\nfoo bar", bytes(range(256)), b"x y z\n"]
    files = []
    for i, p in enumerate(parts):
        f = tmp_path / f"s{i}"
        f.write_bytes(p)
        files.append(str(f))
    on = dataclasses.replace(splitmod.TUNABLES, pack_input=True)
    off = dataclasses.replace(splitmod.TUNABLES, pack_input=False)
    assert type(on).from_env({"MR_PACK_INPUT": "0"}).pack_input is False and type(on).from_env({}).pack_input is True

    def store(tun, from_files):
        monkeypatch.setattr(splitmod, "TUNABLES", tun)
        st = SplitStore.from_files(files, pin=False, threads=3) if from_files else SplitStore(parts, pin=False)
        st._pinned = True  # a pinned store wants the packed copy (no GPU here: the memory itself is pageable)
        monkeypatch.setattr(mio, "pinned_empty", lambda n: torch.empty(n, dtype=torch.uint8))
        assert st.packed is None  # nothing packs before or during loading
        st.finish_loading()
        return st

    for from_files in (False, True):
        st = store(on, from_files)
        raw = st.buffer.numpy().copy()
        assert bytes(raw) == b"aaaa\nhello world\nfoo bar\n" + bytes(range(256)) + b"\nx y z\n"
        pk = st.packed
        assert list(pk.k) == [1, 4, 8, 3]
        for i in (0, 1, 3):
            a, b = st.region(i, i + 1)
            got = decode(pk.buffer.numpy()[int(pk.offsets[i]):int(pk.offsets[i] + pk.nbytes[i])], int(pk.k[i]), b - a,
                         pk.tables[i])
            assert np.array_equal(got, raw[a:b])
        first = pk.buffer
        st.finish_loading()
        assert st.packed.buffer is first  # packed once
        assert st.newline_counts(0, 4) == [1, 2, 2, 1]
        st0 = store(off, from_files)
        assert st0.packed is None and np.array_equal(st0.buffer.numpy(), raw)
    plain = SplitStore(parts, pin=False)
    plain.finish_loading()
    assert plain.packed is None  # an unpinned store ships nothing: no packed copy
