"""``hbm`` storage, list maps (MRL1 files): written and merged on the device.

CPU: the numpy codec (``codec.encode_lists`` / ``decode_lists``, the kernels'
specification) and its reading as records, the descriptors of staged and
device-written files, the routing decision (``job._hbm_route_lists``), the
host guard in front of the decode kernel (``job._check_mrl1_layout``), the
write decision (``device.mrl1_file_plan``), the knob's default, a host merge
over MRL1 and MRK1 files of one partition.

CPU and GPU: ``job._reduce_list_rows`` over three overlapping files against
``utils.merge_iterator`` over the same files written as MRK1 records.

GPU: the same list map through ``job._run_generic_map`` with
``MR_HBM_DEVICE_WRITE`` on and off; whole jobs (examples/LatencyStats through
``device_reducefn``, a ``gen_modules`` list mode through its host reducefn)
that stage no byte of their map files and read none back to the host.
"""
import dataclasses
import importlib
import os
import struct
import sys
import types

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from lua_mapreduce_1_amd import utils  # noqa: E402
from lua_mapreduce_1_amd.ops import _hip  # noqa: E402
from lua_mapreduce_1_amd.ops import keys as K  # noqa: E402
from lua_mapreduce_1_amd.parallel import generic as G  # noqa: E402
from lua_mapreduce_1_amd.runtime import codec, coordinator, device as dev, hbm_store, job as job_mod  # noqa: E402
from lua_mapreduce_1_amd.utils import config  # noqa: E402

NPDT = {0: np.int64, 1: np.float64}


# -- building list files in Python --------------------------------------------------------------
def _mrl1(keys: list[bytes], lists: list[list], code: int) -> bytes:
    """An MRL1 file of the sorted ``keys`` (pack_key under the current hash mask) and their lists."""
    packed = [K.pack_key(w) for w in keys]
    n = len(keys)
    off = np.zeros(n + 1, np.int64)
    np.cumsum([len(w) for w in keys], out=off[1:])
    loff = np.zeros(n + 1, np.int64)
    np.cumsum([len(v) for v in lists], out=loff[1:])
    blob = np.frombuffer(b"".join(keys), np.uint8) if keys else np.zeros(0, np.uint8)
    val = np.array([x for v in lists for x in v], NPDT[code])
    return codec.encode_lists(np.array([p[0] for p in packed], np.uint64).reshape(n),
                              np.array([p[1] for p in packed], np.uint64).reshape(n), off, blob, loff, val, code)


def _mrk1(keys: list[bytes], lists: list[list]) -> bytes:
    return codec.encode_records((codec.key_str(k), list(v)) for k, v in zip(keys, lists))


def _small(n: int, code: int = 0, seed: int = 0):
    """(keys, lists) of n sorted keys; every third list empty, the others of 1..5 values."""
    rng = np.random.default_rng(seed)
    keys = sorted({rng.integers(97, 123, int(rng.integers(1, 30))).astype(np.uint8).tobytes()
                   for _ in range(3 * n)})[:n]
    assert len(keys) == n
    lists = []
    for i in range(n):
        m = 0 if i % 3 == 2 else int(rng.integers(1, 6))
        v = rng.integers(-(1 << 40), 1 << 40, m)
        lists.append([int(x) for x in v] if code == 0 else [float(x) / 8 for x in v])
    return keys, lists


def _head(b: bytes):
    h = hbm_store.mrl1_header(b)
    return h["rows"], h["nb"], h["nv"], h["code"]


def _layout(files):
    lens = [len(b) for b in files]
    bases, total = job_mod._aligned_bases(lens)
    heads = [_head(b) for b in files]
    return total, bases, [h[0] for h in heads], lens, [h[1] for h in heads], [h[2] for h in heads]


# -- CPU: the codec --------------------------------------------------------------------------------
def test_encode_lists_round_trip():
    z64, zi = np.zeros(0, np.uint64), np.zeros(1, np.int64)
    empty = codec.encode_lists(z64, z64, zi, np.zeros(0, np.uint8), zi, np.zeros(0, np.int64), 0)
    assert len(empty) == 52 and empty[:4] == b"MRL1"
    assert struct.unpack("<QQQQ", empty[4:36]) == (0, 0, 0, 0)
    c = codec.decode_lists(empty)
    assert c["hi"].size == 0 and c["list_off"].tolist() == [0] and c["key_off"].tolist() == [0]
    assert list(codec.decode_records(empty)) == []
    # every list empty
    keys = [b"a", b"bb", b"a-key-longer-than-fifteen-bytes"]
    b = _mrl1(keys, [[], [], []], 0)
    assert len(b) == 52 + 32 * 3 + sum(map(len, keys)) and _head(b) == (3, sum(map(len, keys)), 0, 0)
    assert list(codec.decode_records(b)) == [(codec.key_str(k), []) for k in keys]
    # f64 bits: NaN payloads, signed zeros, infinities survive; the bytes are the layout the docstring gives
    bits = np.array([0x7FF80000DEADBEEF, 0x8000000000000000, 0, 0x7FF0000000000000, 0xFFF0000000000000, 1], np.uint64)
    hi = np.array([5, 6, 7], np.uint64)
    lo = np.array([8, 9, 10], np.uint64)
    koff = np.array([0, 1, 3, 6], np.int64)
    blob = np.frombuffer(b"abbccc", np.uint8)
    loff = np.array([0, 0, 5, 6], np.int64)
    for val in (bits, bits.view(np.float64)):
        f = codec.encode_lists(hi, lo, koff, blob, loff, val, 1)
        assert f == (b"MRL1" + struct.pack("<QQQQ", 3, 6, 6, 1) + hi.tobytes() + lo.tobytes() + koff.tobytes()
                     + loff.tobytes() + bits.tobytes() + b"abbccc")
        assert len(f) == 52 + 32 * 3 + 8 * 6 + 6
        c = codec.decode_lists(f)
        assert c["code"] == 1 and c["list_val"].dtype == np.float64
        assert np.array_equal(c["list_val"].view(np.uint64), bits)
        assert np.array_equal(c["hi"], hi) and np.array_equal(c["lo"], lo)
        assert np.array_equal(c["key_off"], koff) and np.array_equal(c["list_off"], loff)
        assert c["key_blob"].tobytes() == b"abbccc"
    i = codec.decode_lists(codec.encode_lists(hi, lo, koff, blob, loff, bits.view(np.int64), 0))
    assert i["list_val"].dtype == np.int64 and np.array_equal(i["list_val"].view(np.uint64), bits)
    with pytest.raises(ValueError):
        codec.encode_lists(hi, lo, koff, blob, loff, bits, 2)
    with pytest.raises(ValueError):
        codec.encode_lists(hi, lo, koff, blob, loff, bits[:5], 0)  # list_off[n] != nv
    with pytest.raises(ValueError):
        codec.decode_lists(f[:-1])
    with pytest.raises(ValueError):
        codec.decode_lists(_mrk1([b"a"], [[1]]))


@pytest.mark.parametrize("code", [0, 1])
def test_decode_records_reads_mrl1_as_the_mrk1_records(code):
    keys, lists = _small(40, code, 3)
    keys += [b"caf\xc3\xa9", b"\xff\xfe"]
    lists += [[1] if code == 0 else [1.5], []]
    a = list(codec.decode_records(_mrl1(keys, lists, code)))
    b = list(codec.decode_records(_mrk1(keys, lists)))
    assert a == b and len(a) == 42
    assert all(type(x) is type(y) for (_k, v), (_q, w) in zip(a, b) for x, y in zip(v, w))


def test_mrl1_header_of_a_blob():
    keys, lists = _small(9, 1, 1)
    b = _mrl1(keys, lists, 1)
    n, nb, nv, code = _head(b)
    assert (n, nv, code) == (9, sum(map(len, lists)), 1) and len(b) == 52 + 32 * n + 8 * nv + nb
    assert hbm_store.mrl1_header(_mrk1(keys, lists)) is None
    assert hbm_store.mrl1_header(b"MRL1") is None and hbm_store.mrl1_header(b"") is None
    assert hbm_store.mrl1_header(b[:35]) is None
    assert hbm_store.mrc2_header(b) is None
    mrc1 = codec.encode_columnar(np.zeros(3, np.uint64), np.zeros(3, np.uint64), np.zeros(3, np.int64),
                                 np.zeros(4, np.int64), np.zeros(0, np.uint8))
    assert hbm_store.mrl1_header(mrc1) is None


# -- CPU: descriptors and routes -----------------------------------------------------------------
@pytest.fixture
def cpu_store(monkeypatch, tmp_path):
    monkeypatch.setattr(dev, "default_device", lambda: torch.device("cpu"))
    monkeypatch.setenv("MR_HBM_SHM_DIR", str(tmp_path))
    st = hbm_store.HBMStore()
    monkeypatch.setattr(hbm_store, "_STORE", st)
    try:
        yield st
    finally:
        st.release()


def test_put_many_and_publish_give_equal_descriptors(cpu_store):
    st = cpu_store
    files = [_mrl1(*_small(1, 0, 1), 0), _mrl1(*_small(300, 1, 2), 1), _mrl1([b"k"], [[]], 0), b"not columnar",
             _mrk1(*_small(4, 0, 3))]
    names = [f"/x/map_results.P{i}.M1" for i in range(len(files))]
    sizes = [len(b) for b in files]
    ml = [hbm_store.mrl1_header(b) for b in files]
    assert [m is not None for m in ml] == [True, True, True, False, False]
    places = st.reserve_many(sizes, gen=("db", 1))
    for pl, b in zip(places, files):
        m = pl.mem
        m[:] = b
        del m
    before = dict(st.stats)
    pub = st.publish(names, places, sizes, [-1] * 5, [-1] * 5, plan_bytes=8 * (3 * 5 + 3), mrl1=ml)
    assert st.stats["dev_puts"] - before["dev_puts"] == len(files)
    assert st.stats["plan_bytes"] - before["plan_bytes"] == 144
    put = st.put_many(list(zip(names, files)), gen=("db", 1))
    for (_n, a), (_m, b), f in zip(pub, put, files):
        a, b = hbm_store.HBMStore.parse(a), hbm_store.HBMStore.parse(b)
        assert sorted(a) == sorted(b) and ("mrl1" in a) == (f[:4] == b"MRL1") and "mrc2" not in a
        assert {k: v for k, v in a.items() if k not in ("off", "c", "h")} == \
               {k: v for k, v in b.items() if k not in ("off", "c", "h")}
        assert (a["rows"], a["nb"]) == (-1, -1)
        if "mrl1" in a:
            assert (a["mrl1"]["rows"], a["mrl1"]["nb"], a["mrl1"]["nv"], a["mrl1"]["code"]) == _head(f)
    assert [st.read_bytes(x) for _n, x in pub] == files == [st.read_bytes(x) for _n, x in put]
    assert st.read_many([x for _n, x in pub]) == files
    with pytest.raises(ValueError):
        st.publish(names, places, sizes, [-1] * 5, [-1] * 5, mrl1=ml[:2])


def test_route_pulls_only_all_mrl1_sets_of_one_code(cpu_store):
    st = cpu_store
    di = [x for _n, x in st.put_many([(f"i{i}", _mrl1(*_small(4 + i, 0, i), 0)) for i in range(3)])]
    df = [x for _n, x in st.put_many([(f"f{i}", _mrl1(*_small(4 + i, 1, i), 1)) for i in range(2)])]
    drec = [x for _n, x in st.put_many([("r", _mrk1(*_small(3, 0, 9)))])]
    d2 = [x for _n, x in st.put_many([("c", codec.encode_columns(np.zeros(1, np.uint64), np.zeros(1, np.uint64),
                                                                 [np.zeros(1, np.int64)], np.array([0, 1], np.int64),
                                                                 np.zeros(1, np.uint8)))])]
    assert job_mod._hbm_route_lists(di, True) == "pull" and job_mod._hbm_route_lists(df, True) == "pull"
    assert job_mod._hbm_route_lists(di[:1], True) == "pull"
    assert job_mod._hbm_route_lists(di, False) == "read"  # a CPU reader
    assert job_mod._hbm_route_lists([], True) == "read"
    for mix in (di + drec, drec + di, drec, di[:1] + drec + di[1:], di + df, df + di, di + d2, d2):
        assert job_mod._hbm_route_lists(mix, True) == "read"
    # the other routes never take an MRL1 file
    assert job_mod._hbm_route(di, True, True) == "read" and job_mod._hbm_route_cols(di, True) == "read"


def test_check_mrl1_layout_accepts_what_the_encoder_writes():
    for code in (0, 1):
        files = [_mrl1(*_small(5, code, 1), code), _mrl1(*_small(40, code, 2), code), _mrl1([b"k", b"l"], [[], []], code),
                 _mrl1(*_small(3, code, 3), code)]
        total, bases, rows, lens, nbs, nvs = _layout(files)
        assert all(52 + 32 * n + 8 * nv + nb == ln for n, nb, nv, ln in zip(rows, nbs, nvs, lens))
        job_mod._check_mrl1_layout(total, bases, rows, lens, nbs, nvs)
    job_mod._check_mrl1_layout(16, [], [], [], [], [])


@pytest.mark.parametrize("what", ["rows<0", "nb<0", "nv<0", "truncated", "padded", "rows+1", "rows-1", "nb+1", "nv+1",
                                  "nv-1", "huge_rows", "huge_nv", "values_without_rows", "outside", "negative_base",
                                  "base_0_mod_8", "base_6_mod_8", "lists_differ"])
def test_check_mrl1_layout_refuses(what, monkeypatch):
    """Every case is refused with ValueError before anything is allocated or
    launched (``_decode_list_files`` reaches no native call)."""
    files = [_mrl1(*_small(5, 0, 1), 0), _mrl1(*_small(41, 0, 2), 0), _mrl1(*_small(3, 0, 3), 0)]
    total, bases, rows, lens, nbs, nvs = _layout(files)
    if what == "rows<0":
        rows[1] = -1
    elif what == "nb<0":
        nbs[1] = -1
    elif what == "nv<0":
        nvs[1] = -1
    elif what == "truncated":
        lens[1] -= 1
    elif what == "padded":
        lens[1] += 1
    elif what == "rows+1":
        rows[1] += 1
    elif what == "rows-1":
        rows[1] -= 1
    elif what == "nb+1":
        nbs[1] += 1
    elif what == "nv+1":
        nvs[1] += 1
    elif what == "nv-1":
        nvs[1] -= 1
    elif what == "huge_rows":
        rows[1] = 2**59 + rows[1]  # 32 n wraps to the same value in 64-bit arithmetic
    elif what == "huge_nv":
        nvs[1] = 2**61 + nvs[1]
    elif what == "values_without_rows":
        rows[1], nvs[1] = 0, nvs[1] + 4 * rows[1]  # the same length
    elif what == "outside":
        total = bases[2] + lens[2] - 1
    elif what == "negative_base":
        bases[0] = -4
    elif what == "base_0_mod_8":
        bases[1] += 4
    elif what == "base_6_mod_8":
        bases[1] += 2
    elif what == "lists_differ":
        nvs = nvs[:2]
    with pytest.raises(ValueError, match="MRL1 decode"):
        job_mod._check_mrl1_layout(total, bases, rows, lens, nbs, nvs)

    def boom(*a, **k):
        raise AssertionError("reached a native call")
    monkeypatch.setattr(_hip, "call", boom)
    monkeypatch.setattr(_hip, "lib", boom)
    with pytest.raises(ValueError, match="MRL1 decode"):
        job_mod._decode_list_files(torch.zeros(total, dtype=torch.uint8), bases, rows, lens, nbs, nvs)


def test_device_write_decision_for_list_maps():
    rows = np.array([3, 0, 2, 0], np.int64)
    nbs = np.array([10, 0, 7, 0], np.int64)
    nvs = np.array([4, 0, 0, 0], np.int64)

    def plan(total_nb=17, total_nv=4, nrows=5, r=rows, b=nbs, v=nvs):
        return np.concatenate([r, b, v, [total_nb, total_nv, nrows]]).astype(np.int64)

    parts, starts, r, b, v, sizes = dev.mrl1_file_plan(plan(), 5, 4, 17, 4)
    assert (parts.tolist(), starts.tolist(), r.tolist(), b.tolist(), v.tolist()) == ([0, 2], [0, 3], [3, 2], [10, 7],
                                                                                    [4, 0])
    assert sizes.tolist() == [52 + 32 * 3 + 8 * 4 + 10, 52 + 32 * 2 + 7]
    assert dev.mrl1_file_plan(plan(), 5, 4, 20, 9) is not None           # a blob / value buffer with room to spare
    assert dev.mrl1_file_plan(plan(nrows=6), 5, 4, 17, 4) is None        # the counts are not the n rows
    assert dev.mrl1_file_plan(plan(nrows=4), 5, 4, 17, 4) is None
    assert dev.mrl1_file_plan(plan(total_nb=18), 5, 4, 18, 4) is None    # ... nor the key bytes
    assert dev.mrl1_file_plan(plan(total_nv=5), 5, 4, 17, 5) is None     # ... nor the values
    assert dev.mrl1_file_plan(plan(), 5, 4, 16, 4) is None               # off[n] past the blob
    assert dev.mrl1_file_plan(plan(), 5, 4, 17, 3) is None               # list_off[n] past list_val
    assert dev.mrl1_file_plan(plan(total_nb=-1), 5, 4, 17, 4) is None
    assert dev.mrl1_file_plan(plan(total_nv=-1), 5, 4, 17, 4) is None
    neg = nvs.copy()
    neg[0], neg[1] = 5, -1
    assert dev.mrl1_file_plan(plan(v=neg), 5, 4, 17, 4) is None
    negb = nbs.copy()
    negb[0], negb[1] = 11, -1
    assert dev.mrl1_file_plan(plan(b=negb), 5, 4, 17, 4) is None


def test_knob_default_is_unchanged():
    assert config.Tunables.from_env({}).hbm_device_write is True
    assert config.Tunables.from_env({"MR_HBM_DEVICE_WRITE": "0"}).hbm_device_write is False


# -- three overlapping files of one partition ------------------------------------------------------
NFILES = 3


def _words() -> list[bytes]:
    """~500 distinct keys: packed ones of every length 1..15, long ones that
    share 8- and 16-byte prefixes over a tiny alphabet (they collide once the
    long-key hash is cut), a few very long."""
    rng = np.random.default_rng(11)
    seen: set = set()
    for n in range(1, 16):
        for _ in range(10):
            seen.add(rng.integers(97, 123, n).astype(np.uint8).tobytes())
    seen.update((b"a", b"prefixAA", b"prefixAAprefixA", b"prefixAAprefixAA"))
    prefixes = [b"prefixAA", b"prefixAB", b"zzzzzzzz", b"prefixAAprefixAA", b"prefixAAprefixAB"]
    while len(seen) < 500:
        p = prefixes[int(rng.integers(0, len(prefixes)))]
        n = int(rng.integers(8, 40)) if rng.random() < 0.98 else int(rng.integers(200, 400))
        seen.add(p + rng.integers(97, 100, n).astype(np.uint8).tobytes())
    return sorted(seen)


WORDS = _words()
ONLY_ONE = b"empty-in-one-file-only"       # (>= 16 bytes: a long key)
EVERYWHERE = b"empty-everywhere"


def _make_files(code: int):
    """Per file (keys, lists): overlapping sorted key sets; a key with an
    empty list in the second file only, one with an empty list in all files,
    others with an empty list in one file and values in another."""
    rng = np.random.default_rng(5 + code)
    out = []
    for f in range(NFILES):
        pick = set(w for w in WORDS if rng.random() < 0.6)
        pick.add(EVERYWHERE)
        if f == 1:
            pick.add(ONLY_ONE)
        keys = sorted(pick)
        lists = []
        for k in keys:
            m = 0 if k in (EVERYWHERE, ONLY_ONE) or rng.random() < 0.15 else int(rng.integers(1, 7))
            v = rng.integers(-(1 << 50), 1 << 50, m)
            lists.append([int(x) for x in v] if code == 0 else [float(x) / 16 for x in v])
        out.append((keys, lists))
    return out


@pytest.fixture
def on_device(request, monkeypatch, tmp_path):
    name = request.param
    if name == "cuda":
        request.getfixturevalue("gpu")
        d = torch.device("cuda", 0)
    else:
        d = torch.device("cpu")
    monkeypatch.setattr(dev, "default_device", lambda: d)
    monkeypatch.setenv("MR_HBM_SHM_DIR", str(tmp_path))
    st = hbm_store.HBMStore()
    monkeypatch.setattr(hbm_store, "_STORE", st)
    try:
        yield d
    finally:
        st.release()


def _host_merge(blobs: list[bytes]) -> list:
    names = [f"f{i}" for i in range(len(blobs))]
    by = dict(zip(names, blobs))
    return list(utils.merge_iterator(None, names, lambda n: codec.decode_records(by[n])))


def _rows_of(files: list[bytes], d):
    """What mr_mrl1_decode gives for the files, from the numpy decoder: the
    files laid out at 4 mod 16 in one buffer, rep words into it."""
    bases, total = job_mod._aligned_bases([len(b) for b in files])
    host = np.zeros(max(total, 16), np.uint8)
    hi, lo, rep, vbits, vrow, r0 = [], [], [], [], [], 0
    for o, b in zip(bases, files):
        host[o:o + len(b)] = np.frombuffer(b, np.uint8)
        c = codec.decode_lists(b)
        n = int(c["hi"].size)
        kb = o + len(b) - int(c["key_blob"].size)
        ko = c["key_off"]
        hi.append(c["hi"])
        lo.append(c["lo"])
        rep += [K.make_rep(kb + int(ko[i]), int(ko[i + 1] - ko[i])) for i in range(n)]
        vbits.append(c["list_val"].view(np.int64))
        vrow.append(np.repeat(np.arange(n, dtype=np.int64), np.diff(c["list_off"])) + r0)
        r0 += n
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(d)  # noqa: E731
    buf = t(host)
    return (t(np.concatenate(hi).view(np.int64)), t(np.concatenate(lo).view(np.int64)),
            t(np.array(rep, np.uint64).view(np.int64)), buf, t(np.concatenate(vbits)), t(np.concatenate(vrow)))


@pytest.mark.parametrize("code", [0, 1], ids=["i64", "f64"])
@pytest.mark.parametrize("collide", [False, True], ids=["hash56", "hash2"])
@pytest.mark.parametrize("on_device", ["cpu", pytest.param("cuda", marks=pytest.mark.gpu)], indirect=True)
def test_reduce_list_rows_matches_merge_iterator(on_device, collide, code, monkeypatch):
    """Keys, and every list's exact order (files in order, then file order),
    as the heap merge over the same files written as MRK1 gives them; empty
    lists kept.  With the long-key hash cut to 2 bits distinct long keys meet
    on (hi, lo) and only their bytes tell them apart.  On the GPU the rows
    come from mr_mrl1_decode over files pulled from the store."""
    gpu = on_device.type == "cuda"
    dtype = job_mod._MRL1_DTYPE[code]
    try:
        if collide:
            K.set_long_hash_bits(2)
        parts = _make_files(code)
        files = [_mrl1(k, v, code) for k, v in parts]
        want = _host_merge([_mrk1(k, v) for k, v in parts])
        assert _host_merge(files) == want
        wd = dict(want)
        assert wd[codec.key_str(ONLY_ONE)] == [] and wd[codec.key_str(EVERYWHERE)] == []
        assert sum(1 for k in parts[0][0] if len(k) > K.PACK_MAX) > 50
        if collide:
            owners = {}
            for b in files:
                c = codec.decode_lists(b)
                for h, l, i in zip(c["hi"].tolist(), c["lo"].tolist(), range(c["hi"].size)):
                    if K.is_long(l):
                        owners.setdefault((h, l), set()).add(c["key_blob"][c["key_off"][i]:c["key_off"][i + 1]].tobytes())
            assert any(len(s) > 1 for s in owners.values())
        if gpu:
            st = hbm_store.store()
            descs = [x for _n, x in st.put_many([(f"red.P0.M{i}", b) for i, b in enumerate(files)])]
            assert job_mod._hbm_route_lists(descs, True) == "pull"
            calls = []
            real = hbm_store.HBMStore.read_many
            monkeypatch.setattr(hbm_store.HBMStore, "read_many", lambda self, d: calls.append(1) or real(self, d))
            before = st.stats["pulls"]
            buf, bases, ds = st.pull_device(descs, on_device)
            ml = [x["mrl1"] for x in ds]
            hi, lo, rep, vbits, vrow = job_mod._decode_list_files(
                buf, bases, [m["rows"] for m in ml], [x["len"] for x in ds], [m["nb"] for m in ml],
                [m["nv"] for m in ml])
            assert st.stats["pulls"] - before == NFILES and not calls
            w = _rows_of(files, on_device)
            for g, e in zip((hi, lo, rep, vbits, vrow), (w[0], w[1], w[2], w[4], w[5])):
                assert torch.equal(g, e)
            src = buf
        else:
            hi, lo, rep, src, vbits, vrow = _rows_of(files, on_device)
        out = job_mod._reduce_list_rows(hi, lo, rep, src, vbits, vrow, dtype)
        got = list(codec.iter_columnar(G.host_partitions(out, 1, dtype)[0]))
        assert [k for k, _ in got] == [k for k, _ in want]
        assert got == want
        assert all(type(x) is type(y) for (_k, v), (_q, u) in zip(got, want) for x, y in zip(v, u))
        # the records of the whole route: a per-key reducer that keeps the order visible
        recs = job_mod._list_records(out, None, lambda k, v, emit: [emit(x) for x in v], False, False, dtype)
        assert recs == want
    finally:
        K.set_long_hash_bits(None)


def test_host_merge_of_half_mrl1_half_mrk1_files(cpu_store):
    """One partition whose files are MRL1 (a device map) and MRK1 (a host map,
    or a map whose plan was rejected) side by side, read through the store as
    a CPU reducer does: the all-MRK1 merge."""
    from lua_mapreduce_1_amd.runtime import fs as fsmod
    st = cpu_store
    for code in (0, 1):
        parts = _make_files(code) + _make_files(code)[:1]
        all_rec = [_mrk1(k, v) for k, v in parts]
        mixed = [_mrl1(k, v, code) if i % 2 == 0 else _mrk1(k, v) for i, (k, v) in enumerate(parts)]
        want = _host_merge(all_rec)
        assert _host_merge(mixed) == want
        names = [f"/p/map_results.P0.M{i}" for i in range(len(mixed))]
        descs = dict(st.put_many(list(zip(names, mixed)), gen=("mix", code)))
        assert job_mod._hbm_route_lists([descs[n] for n in names], True) == "read"
        assert st.read_many([descs[n] for n in names]) == mixed

        class Cnn:
            def gridfs(self):
                return types.SimpleNamespace(get=lambda n: descs.get(n))
        m, _b, lines = fsmod.router(Cnn(), None, "hbm", "/p")
        assert list(utils.merge_iterator(m, names, lines)) == want


# -- GPU: the same map both ways ------------------------------------------------------------------
class _Files:
    def __init__(self):
        self.items = []

    def store_many(self, items):
        self.items.extend(items)
        return True


def _map_job(value, nparts: int, files: _Files, module: dict):
    """A map job object with just what ``_run_generic_map`` uses: the
    coordinator's blob store is ``files``, the job table a stub."""
    class Cnn:
        dbname = "hbm_lists_device"

        def gridfs(self):
            return files

    class Jobs:
        def update(self, *a, **k):
            return {}

    j = job_mod.job.__new__(job_mod.job)
    j.cnn, j.jobs = Cnn(), Jobs()
    j.job_tbl = {"_id": 1, "value": value}
    j.task_tbl = {"iteration": 1, "extra": {"num_partitions": nparts, "table_capacity": 1 << 12}}
    j.storage, j.path, j.results_ns = "hbm", "/tmp/hbm_lists_device", "map_results"
    j.module = module
    j.t, j.written = utils.time(), False
    return j


def _set_knob(monkeypatch, on: bool) -> None:
    monkeypatch.setattr(config, "TUNABLES", dataclasses.replace(config.TUNABLES, hbm_device_write=on))


def _concat_map(key, value, emit):
    from lua_mapreduce_1_amd.ops import text as TX
    ks, kl, (v,) = TX.csv_rows(value, 0, (1,), ",")
    emit.spans(ks, kl, (v * 8).to(torch.int64), text=value)


def _csv() -> bytes:
    """A few thousand ``key,score`` rows over a few hundred keys (some longer
    than 15 bytes, up to 240), every score a multiple of 1/8."""
    rng = np.random.default_rng(21)
    letters = np.frombuffer(b"abcdefghijklmnopqrstuvwxyz", np.uint8)
    keys = sorted({rng.choice(letters, int(rng.integers(1, 16))).tobytes() for _ in range(260)})
    keys += [b"L%03dxyzw" % i + b"tail" * int(rng.integers(2, 14)) for i in range(40)]
    keys += [b"prefixAAprefixAA" + rng.choice(letters[:3], int(rng.integers(1, 30))).tobytes() for _ in range(30)]
    keys += [b"very-long-" + rng.choice(letters, 230).tobytes()]
    keys = sorted(set(keys))
    lines = []
    for _ in range(5000):
        k = keys[int(rng.integers(0, len(keys)))]
        lines.append(k + b"," + (b"%.3f" % (int(rng.integers(0, 1 << 17)) / 8)))
    return b"\n".join(lines) + b"\n"


def _latency_map():
    return importlib.import_module("lua_mapreduce_1_amd.examples.LatencyStats").device_mapfn


# module of the map job, device_reduce of the reduce module, the value code, the knob-off host encoding
MAPS = {
    "concat": (lambda: {"device_mapfn": _concat_map, "device_value_dtype": "i64"}, "concat", 0),
    "concat_unique": (lambda: {"device_mapfn": _concat_map, "device_value_dtype": "i64"}, "concat_unique", 0),
    "latency": (lambda: {"device_mapfn": _latency_map(), "device_value_dtype": "f64"}, "concat", 1),
}


def _run_map(text, nparts: int, which: str):
    module, op, _code = MAPS[which]
    st = hbm_store.store()
    files = _Files()
    before = dict(st.stats)
    outs = []
    real = G.order_lists
    try:
        G.order_lists = lambda *a, **k: outs.append(real(*a, **k)) or outs[-1]
        with dev.PLANE_LOCK:
            _map_job(text, nparts, files, module())._run_generic_map(
                types.SimpleNamespace(device_partition=("fnv1", nparts)), types.SimpleNamespace(device_reduce=op),
                "list")
    finally:
        G.order_lists = real
    delta = {k: st.stats[k] - before[k] for k in before}
    descs = [(n, b) for n, b in files.items if hbm_store.is_descriptor(b)]
    index = sorted(n for n, b in files.items if not hbm_store.is_descriptor(b))
    assert descs and len(index) == len(descs) and delta["puts"] == len(descs)
    got = {n: (st.read_bytes(b), {k: v for k, v in hbm_store.HBMStore.parse(b).items() if k not in ("off", "c", "h")})
           for n, b in descs}
    assert len(outs) == 1
    return got, index, delta, outs[0]


@pytest.mark.gpu
@pytest.mark.parametrize("nparts", [1, 6, 256])
@pytest.mark.parametrize("which", list(MAPS))
def test_same_list_map_with_the_knob_on_and_off(gpu, monkeypatch, which, nparts):
    text = torch.frombuffer(bytearray(_csv()), dtype=torch.uint8).to(gpu)
    _module, _op, code = MAPS[which]
    dtype = job_mod._MRL1_DTYPE[code]
    got = {}
    for on in (True, False):
        _set_knob(monkeypatch, on)
        got[on], got[on, "index"], delta, out = _run_map(text, nparts, which)
        if on:
            # the device path ran (else the comparison below shows nothing)
            assert delta["dev_puts"] == delta["puts"] > 0 and delta["staged_bytes"] == 0
            assert delta["plan_bytes"] == 8 * (3 * nparts + 3)
            host = G.host_partitions(out, nparts, dtype)
        else:
            assert delta["dev_puts"] == 0 and delta["plan_bytes"] == 0
            assert delta["staged_bytes"] == delta["put_bytes"] > 0
    assert sorted(got[True]) == sorted(got[False]) and got[True, "index"] == got[False, "index"]
    assert len(got[True]) == len(host)
    seen = set()
    for p, cols in host.items():
        name = f"/tmp/hbm_lists_device/map_results.P{p}.M1"
        blob, d = got[True][name]
        # byte for byte the numpy codec over the host slice
        assert blob == codec.encode_lists(cols["hi"], cols["lo"], cols["key_off"], cols["key_blob"], cols["list_off"],
                                          cols["list_val"], code), name
        assert (d["rows"], d["nb"]) == (-1, -1) and "mrc2" not in d
        assert (d["mrl1"]["rows"], d["mrl1"]["nb"], d["mrl1"]["nv"], d["mrl1"]["code"]) == _head(blob)
        assert d["mrl1"]["code"] == code and d["len"] == len(blob)
        # ... and the records of the knob-off file (MRK1), whose descriptor has no counts
        off_blob, off_d = got[False][name]
        assert off_blob[:4] == b"MRK1" and "mrl1" not in off_d
        recs = list(codec.decode_records(blob))
        assert recs == list(codec.decode_records(off_blob)) and recs
        keys = [k for k, _ in recs]
        assert all(a.encode("utf-8", "surrogateescape") < b.encode("utf-8", "surrogateescape")
                   for a, b in zip(keys, keys[1:])), name
        assert not seen & set(keys)
        seen |= set(keys)
    assert len(seen) > 300


@pytest.mark.gpu
def test_a_rejected_list_plan_falls_back_to_the_same_files(gpu, monkeypatch):
    """The lists are ordered on the device when the plan is rejected (here:
    every plan): the host encoder then writes the same ``out`` — the MRK1
    files of the knob-off run, all of them staged, nothing reserved."""
    text = torch.frombuffer(bytearray(_csv()), dtype=torch.uint8).to(gpu)
    got = {}
    for reject in (True, False):
        _set_knob(monkeypatch, reject)  # knob on with every plan rejected, then knob off
        seen, reserved = [], []
        real = dev.mrl1_file_plan
        real_reserve = hbm_store.HBMStore.reserve_many

        def plan(*a, **k):
            seen.append(real(*a, **k) is not None)
            return None

        monkeypatch.setattr(dev, "mrl1_file_plan", plan)
        monkeypatch.setattr(hbm_store.HBMStore, "reserve_many",
                            lambda self, *a, **k: reserved.append(1) or real_reserve(self, *a, **k))
        got[reject], _index, delta, _out = _run_map(text, 6, "latency")
        monkeypatch.setattr(dev, "mrl1_file_plan", real)
        monkeypatch.setattr(hbm_store.HBMStore, "reserve_many", real_reserve)
        assert seen == ([True] if reject else [])  # the plan was a good one
        assert not reserved and delta["dev_puts"] == 0 and delta["plan_bytes"] == 0
        assert delta["staged_bytes"] == delta["put_bytes"] > 0
    assert got[True] and got[True] == got[False]
    assert all(b[:4] == b"MRK1" for b, _d in got[True].values())


# -- GPU: whole jobs -----------------------------------------------------------------------------
@pytest.fixture(scope="module")
def cs():
    return coordinator.start_local()


def _in_a_reduce_job() -> bool:
    f = sys._getframe(1)
    while f is not None:
        if f.f_code.co_name == "run" and f.f_code.co_filename == job_mod.__file__:
            return True
        f = f.f_back
    return False


LS = "lua_mapreduce_1_amd.examples.LatencyStats"
GM = "gen_modules"


def _whole_job(cs, tmp_path, which: str, db: str):
    """(result, oracle, server) of a job over hbm storage with 2 worker threads."""
    from test_e2e_wordcount import run_job
    from test_generic_plane import make_data
    from test_generic_server_worker import write
    if which == "latency":
        mod = importlib.import_module(LS)
        splits = mod.make_log(seed=4, lines=20_000, endpoints=50)
        name, args, want = LS, {"num_reducers": 3, "quiet": True}, mod.naive(splits)
    else:
        mod = importlib.import_module(GM)
        splits = make_data("text")[:4]
        name, args, want = GM, {"mode": which}, mod.oracle(splits, which)
    sub = tmp_path / db
    sub.mkdir()
    files = write(sub, splits)
    p = dict(taskfn=name, mapfn=name, partitionfn=name, reducefn=name, finalfn=name,
             init_args=dict(args, files=files), storage="hbm", device="auto")
    _, s = run_job(cs, f"lists_{db}_{which}", p, nworkers=2)
    return mod.RESULT, want, s


@pytest.mark.gpu
@pytest.mark.parametrize("which", ["latency", "docs", "max_host"])
def test_list_job_stages_nothing(gpu, cs, tmp_path, monkeypatch, which):
    """examples/LatencyStats (the batched device_reducefn) and gen_modules
    list modes (a host reducefn per key) over hbm storage with 2 GPU workers
    (threads: one store).  Knob on: every map file is written on the device
    and no reduce job reads one back to the host.  Knob off: the same result,
    staged."""
    from test_generic_plane import close_lists
    st = hbm_store.store()
    calls = []
    real_many, real_one = hbm_store.HBMStore.read_many, hbm_store.HBMStore.read_bytes
    monkeypatch.setattr(hbm_store.HBMStore, "read_many",
                        lambda self, d: calls.append(_in_a_reduce_job()) or real_many(self, d))
    monkeypatch.setattr(hbm_store.HBMStore, "read_bytes",
                        lambda self, d: calls.append(_in_a_reduce_job()) or real_one(self, d))
    rel = 1e-12 if which == "latency" else 1e-9

    _set_knob(monkeypatch, True)
    before = dict(st.stats)
    got, exp, s = _whole_job(cs, tmp_path, which, "on")
    delta = {k: st.stats[k] - before[k] for k in before}
    assert len(exp) > 30 and close_lists(got, exp, rel=rel)
    assert s.last_stats["failed_map_jobs"] == 0 and s.last_stats["failed_red_jobs"] == 0
    assert delta["staged_bytes"] == 0
    assert delta["dev_puts"] > 0 and delta["dev_puts"] == delta["puts"]
    assert delta["plan_bytes"] > 0 and delta["pulls"] == delta["puts"]
    assert not any(calls)
    got_on = {k: list(v) for k, v in got.items()}

    _set_knob(monkeypatch, False)
    del calls[:]
    before = dict(st.stats)
    got_off, exp, s = _whole_job(cs, tmp_path, which, "off")
    delta = {k: st.stats[k] - before[k] for k in before}
    assert close_lists(got_off, exp, rel=rel)
    assert s.last_stats["failed_map_jobs"] == 0 and s.last_stats["failed_red_jobs"] == 0
    assert delta["staged_bytes"] == delta["put_bytes"] > 0 and delta["dev_puts"] == 0 and delta["pulls"] == 0
    assert any(calls)
    if which != "latency":
        assert got_on == {k: list(v) for k, v in got_off.items()}
