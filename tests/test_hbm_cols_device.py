"""``hbm`` storage, typed folds (MRC2 files): written and read on the device.

CPU: the host guard in front of the decode kernel (``job._check_mrc2_layout``),
the routing decision (``job._hbm_route_cols``; an MRC2 descriptor never goes to
the MRC1 decode), the descriptors of staged and device-written files, the
write decision (``device.mrc2_file_plan``), the knob's default.

GPU: the same typed-fold map through ``job._run_generic_map`` with
``MR_HBM_DEVICE_WRITE`` on and off gives byte-identical files; five
overlapping files of one partition reduce to the same result through the
pulled path, through ``read_many`` + ``_device_reduce_cols`` and in a dict
fold; a whole ScoreStats job with the knob on stages no byte of its map files
and reads none of them back to the host.

Device float sums come from atomics in no fixed order: every value here is an
integer below 2^18 (f32) or 2^30 (f64) divided by 8, so the sums are exact in
any order and runs compare bit for bit.
"""
import dataclasses
import os
import sys
import types

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from lua_mapreduce_1_amd import utils  # noqa: E402
from lua_mapreduce_1_amd.ops import _hip  # noqa: E402
from lua_mapreduce_1_amd.ops import agg as A  # noqa: E402
from lua_mapreduce_1_amd.ops import keys as K  # noqa: E402
from lua_mapreduce_1_amd.runtime import codec, coordinator, device as dev, hbm_store, job as job_mod  # noqa: E402
from lua_mapreduce_1_amd.utils import config  # noqa: E402

CODES = {"i64": 0, "f64": 1, "f32": 2}
NPDT = {0: np.int64, 1: np.float64, 2: np.float32}
WIDTH = {0: 8, 1: 8, 2: 4}


# -- building MRC2 files in Python ---------------------------------------------------------------
def _mrc2(keys: list[bytes], cols: list[np.ndarray]) -> bytes:
    """An MRC2 file of the sorted ``keys`` (pack_key under the current hash mask)."""
    packed = [K.pack_key(w) for w in keys]
    off = np.zeros(len(keys) + 1, np.int64)
    np.cumsum([len(w) for w in keys], out=off[1:])
    blob = np.frombuffer(b"".join(keys), np.uint8) if keys else np.zeros(0, np.uint8)
    return codec.encode_columns(np.array([p[0] for p in packed], np.uint64).reshape(len(keys)),
                                np.array([p[1] for p in packed], np.uint64).reshape(len(keys)), cols, off, blob)


def _small(n: int, codes=(2, 1, 0), seed: int = 0) -> bytes:
    rng = np.random.default_rng(seed)
    keys = sorted({rng.integers(97, 123, int(rng.integers(1, 30))).astype(np.uint8).tobytes()
                   for _ in range(3 * n)})[:n]
    assert len(keys) == n
    return _mrc2(keys, [(rng.integers(0, 1 << 17, n) / 8).astype(NPDT[c]) for c in codes])


def _head(b: bytes):
    h = hbm_store.mrc2_header(b)
    return h["rows"], h["nb"], h["codes"]


def _layout(files):
    lens = [len(b) for b in files]
    bases, total = job_mod._aligned_bases(lens)
    heads = [_head(b) for b in files]
    return total, bases, [h[0] for h in heads], lens, [h[1] for h in heads], [h[2] for h in heads]


# -- CPU: the guard ------------------------------------------------------------------------------
def test_mrc2_header_of_a_blob():
    b = _small(9, (2, 1, 0))
    n, nb, codes = _head(b)
    assert (n, codes) == (9, [2, 1, 0]) and len(b) == 44 + 24 * 9 + 9 * 20 + nb
    assert hbm_store.mrc2_header(codec.encode_records([("a", [1])])) is None
    assert hbm_store.mrc2_header(b"MRC2") is None and hbm_store.mrc2_header(b"") is None
    assert hbm_store.mrc2_header(b[:35]) is None
    mrc1 = codec.encode_columnar(np.zeros(3, np.uint64), np.zeros(3, np.uint64), np.zeros(3, np.int64),
                                 np.zeros(4, np.int64), np.zeros(0, np.uint8))
    assert hbm_store.mrc2_header(mrc1) is None
    nine = codec.encode_columns(np.zeros(1, np.uint64), np.zeros(1, np.uint64), [np.zeros(1, np.int64)] * 9,
                                np.zeros(2, np.int64), np.zeros(0, np.uint8))
    assert hbm_store.mrc2_header(nine) is None  # a longer header: not for the device codec


def test_check_mrc2_layout_accepts_what_the_encoder_writes():
    for codes in ((1,), (2,), (2, 1, 0), (2, 2, 0), (2, 0, 1, 2, 2, 1, 0, 2)):
        files = [_small(5, codes, 1), _small(40, codes, 2), _small(3, codes, 3)]
        total, bases, rows, lens, nbs, cs = _layout(files)
        assert all(44 + 24 * n + n * sum(WIDTH[c] for c in codes) + nb == ln for n, nb, ln in zip(rows, nbs, lens))
        job_mod._check_mrc2_layout(total, bases, rows, lens, nbs, cs, list(codes))
    job_mod._check_mrc2_layout(16, [], [], [], [], [], [1])


@pytest.mark.parametrize("what", ["rows<0", "nb<0", "k=0", "k=9", "code=3", "files_differ", "spec_differs",
                                  "spec_shorter", "spec_k=0", "spec_k=9", "spec_code=7", "truncated", "padded",
                                  "rows+1", "rows-1", "nb+1", "nb-8", "huge_rows", "outside", "negative_base",
                                  "base_0_mod_8", "base_6_mod_8", "lists_differ"])
def test_check_mrc2_layout_refuses(what, monkeypatch):
    """Every case is refused with ValueError before anything is allocated or
    launched (``_decode_cols_files`` reaches no native call)."""
    codes = [2, 1, 0]
    files = [_small(5, codes, 1), _small(41, codes, 2), _small(3, codes, 3)]
    total, bases, rows, lens, nbs, cs = _layout(files)
    want = list(codes)
    if what == "rows<0":
        rows[1] = -1
    elif what == "nb<0":
        nbs[1] = -1
    elif what == "k=0":
        cs[1] = []
    elif what == "k=9":
        cs[1] = [0] * 9
    elif what == "code=3":
        cs[1] = [2, 3, 0]
    elif what == "files_differ":
        cs[1] = [2, 0, 1]   # the same widths: only the codes tell
    elif what == "spec_differs":
        want = [2, 0, 1]
    elif what == "spec_shorter":
        want = [2, 1]
    elif what == "spec_k=0":
        want = []
    elif what == "spec_k=9":
        want = [0] * 9
    elif what == "spec_code=7":
        want = [2, 1, 7]
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
    elif what == "nb-8":
        nbs[1] -= 8
    elif what == "huge_rows":
        rows[1] = 2**62 + rows[1]  # 44 n wraps to the same value in 64-bit arithmetic
    elif what == "outside":
        total = bases[2] + lens[2] - 1
    elif what == "negative_base":
        bases[0] = -4
    elif what == "base_0_mod_8":
        bases[1] += 4
    elif what == "base_6_mod_8":
        bases[1] += 2
    elif what == "lists_differ":
        cs = cs[:2]
    with pytest.raises(ValueError, match="MRC2 decode"):
        job_mod._check_mrc2_layout(total, bases, rows, lens, nbs, cs, want)

    def boom(*a, **k):
        raise AssertionError("reached a native call")
    monkeypatch.setattr(_hip, "call", boom)
    monkeypatch.setattr(_hip, "lib", boom)
    with pytest.raises(ValueError, match="MRC2 decode"):
        job_mod._decode_cols_files(torch.zeros(total, dtype=torch.uint8), bases, rows, lens, nbs, cs, want)


# -- CPU: descriptors and routes -----------------------------------------------------------------
@pytest.fixture
def cpu_store(monkeypatch, tmp_path):
    monkeypatch.setattr(dev, "default_device", lambda: torch.device("cpu"))
    monkeypatch.setenv("MR_HBM_SHM_DIR", str(tmp_path))
    st = hbm_store.HBMStore()
    try:
        yield st
    finally:
        st.release()


def _mrc1(n: int) -> bytes:
    return codec.encode_columnar(np.arange(n, dtype=np.uint64), np.arange(n, dtype=np.uint64),
                                 np.arange(n, dtype=np.int64), np.arange(n + 1, dtype=np.int64), np.zeros(n, np.uint8))


def test_route_pulls_only_all_mrc2_sets(cpu_store):
    st = cpu_store
    d2 = [x for _n, x in st.put_many([(f"c{i}", _small(4 + i, (1, 0), i)) for i in range(3)])]
    d1 = [x for _n, x in st.put_many([("m1", _mrc1(5))])]
    drec = [x for _n, x in st.put_many([("r", codec.encode_records([("k", [1])]))])]
    for x, f in zip(d2, range(3)):
        p = hbm_store.HBMStore.parse(x)
        assert (p["rows"], p["nb"]) == (-1, -1)  # "not an MRC1 file"
        assert p["mrc2"]["rows"] == 4 + f and p["mrc2"]["codes"] == [1, 0] and p["mrc2"]["nb"] > 0
    assert "mrc2" not in hbm_store.HBMStore.parse(d1[0]) and "mrc2" not in hbm_store.HBMStore.parse(drec[0])
    assert job_mod._hbm_route_cols(d2, True) == "pull"
    assert job_mod._hbm_route_cols(d2, False) == "read"  # no GPU
    assert job_mod._hbm_route_cols([], True) == "read"
    for mix in (d2 + d1, d1 + d2, d2 + drec, drec, d1, d2[:1] + drec + d2[1:]):
        assert job_mod._hbm_route_cols(mix, True) == "read"
    # the unchanged MRC1 decision never takes an MRC2 file
    assert job_mod._hbm_route(d2, True, True) == "read"
    assert job_mod._hbm_route(d2 + d1, True, True) == "read"
    assert job_mod._hbm_route(d2, False, True) == "read"
    assert job_mod._hbm_route(d1, True, True) == "pull"


def test_put_many_and_publish_give_equal_descriptors(cpu_store):
    st = cpu_store
    files = [_small(1, (2,), 1), _small(300, (2, 1, 0), 2), _small(7, (0, 1), 3), b"not columnar", _mrc1(4)]
    names = [f"/x/map_results.P{i}.M1" for i in range(len(files))]
    sizes = [len(b) for b in files]
    m2 = [hbm_store.mrc2_header(b) for b in files]
    assert [m is not None for m in m2] == [True, True, True, False, False]
    rows = [-1, -1, -1, -1, 4]
    nbs = [-1, -1, -1, -1, 4]
    places = st.reserve_many(sizes, gen=("db", 1))
    for pl, b in zip(places, files):
        m = pl.mem
        m[:] = b
        del m
    before = dict(st.stats)
    pub = st.publish(names, places, sizes, rows, nbs, plan_bytes=56, mrc2=m2)
    assert st.stats["dev_puts"] - before["dev_puts"] == len(files)
    assert st.stats["plan_bytes"] - before["plan_bytes"] == 56
    put = st.put_many(list(zip(names, files)), gen=("db", 1))
    assert [n for n, _ in pub] == [n for n, _ in put] == names
    for (_n, a), (_m, b), f in zip(pub, put, files):
        a, b = hbm_store.HBMStore.parse(a), hbm_store.HBMStore.parse(b)
        assert sorted(a) == sorted(b) and ("mrc2" in a) == (f[:4] == b"MRC2")
        assert {k: v for k, v in a.items() if k not in ("off", "c", "h")} == \
               {k: v for k, v in b.items() if k not in ("off", "c", "h")}
        assert (a["c"], a["off"]) != (b["c"], b["off"])
    assert [st.read_bytes(x) for _n, x in pub] == files == [st.read_bytes(x) for _n, x in put]
    # the earlier call signatures still work
    p2 = st.reserve_many(sizes[3:4], gen=("db", 1))
    assert "mrc2" not in hbm_store.HBMStore.parse(st.publish(names[3:4], p2, sizes[3:4], [-1], [-1])[0][1])
    with pytest.raises(ValueError):
        st.publish(names, places, sizes, rows, nbs, mrc2=m2[:2])


def test_device_write_decision_for_typed_folds():
    rows = np.array([3, 0, 2, 0], np.int64)
    nbs = np.array([10, 0, 7, 0], np.int64)

    def plan(bad=0, err=0, total=17, nrows=5):
        return np.concatenate([rows, nbs, [bad, err, total, nrows]]).astype(np.int64)

    parts, starts, r, b, sizes = dev.mrc2_file_plan(plan(), 5, 4, 17, 20)
    assert (parts.tolist(), starts.tolist(), r.tolist(), b.tolist()) == ([0, 2], [0, 3], [3, 2], [10, 7])
    assert sizes.tolist() == [44 + 24 * 3 + 20 * 3 + 10, 44 + 24 * 2 + 20 * 2 + 7]
    assert dev.mrc2_file_plan(plan(nrows=6), 5, 4, 17, 20) is None   # the counts are not the n rows
    assert dev.mrc2_file_plan(plan(total=18), 5, 4, 17, 20) is None  # ... nor the key bytes
    assert dev.mrc2_file_plan(plan(), 5, 4, 16, 20) is None
    assert dev.mrc2_file_plan(plan(bad=1), 5, 4, 17, 20) is None
    assert dev.mrc2_file_plan(plan(err=1), 5, 4, 17, 20) is None


def test_knob_default_is_unchanged():
    assert config.Tunables.from_env({}).hbm_device_write is True
    assert config.Tunables.from_env({"MR_HBM_DEVICE_WRITE": "0"}).hbm_device_write is False


# -- the reduce side: five overlapping files of one partition -------------------------------------
NFILES = 5
SPEC = ("f32:sum", "f64:mean", "f64:max", "count", "i64:min")
PHYS_CODES = [2, 1, 0, 1, 0]  # f32 sum | f64 sum, i64 count (the mean; the count shares it) | f64 max | i64 min


def _words() -> list[bytes]:
    """~1200 distinct keys: packed ones of every length 1..15, long ones that
    share 8- and 16-byte prefixes over a tiny alphabet, a few very long, a
    few with bytes >= 0x80."""
    rng = np.random.default_rng(11)
    seen: set = set()
    for n in range(1, 16):
        for _ in range(20):
            seen.add(rng.integers(97, 123, n).astype(np.uint8).tobytes())
    seen.update((b"a", b"prefixAA", b"prefixAAprefixA", b"prefixAAprefixAA", b"\xff", b"\xc3\xa9t\xc3\xa9"))
    prefixes = [b"prefixAA", b"prefixAB", b"zzzzzzzz", b"prefixAAprefixAA", b"prefixAAprefixAB",
                b"caf\xc3\xa9\xe2\x82\xac-"]
    while len(seen) < 1200:
        p = prefixes[int(rng.integers(0, len(prefixes)))]
        n = int(rng.integers(8, 40)) if rng.random() < 0.98 else int(rng.integers(200, 400))
        seen.add(p + rng.integers(97, 100, n).astype(np.uint8).tobytes())
    return sorted(seen)


WORDS = _words()


def _make_files():
    """(files, want): five MRC2 map outputs of one partition (the physical
    columns of SPEC) and the dict fold of their rows: key -> the output
    columns [f32 sum, mean, max, count, min] as numpy scalars."""
    assert [CODES[dt] for dt, _op, _i in A.Physical(A.parse_spec(SPEC)).cols] == PHYS_CODES
    rng = np.random.default_rng(5)
    files, acc = [], {}
    for _f in range(NFILES):
        pick = [w for w in WORDS if rng.random() < 0.55]  # overlapping key sets, each sorted
        n = len(pick)
        s32 = (rng.integers(-(1 << 17), 1 << 17, n) / 8).astype(np.float32)
        s64 = rng.integers(-(1 << 29), 1 << 29, n) / 8
        cnt = rng.integers(1, 1000, n).astype(np.int64)
        mx = rng.integers(-(1 << 29), 1 << 29, n) / 8
        mn = rng.integers(-2**63, 2**63 - 1, n, dtype=np.int64, endpoint=True)
        mx[1::43] = -np.inf  # (no signed zeros here: max(-0.0, 0.0) has no one answer)
        mn[::37], mn[1::31] = -2**63, 2**63 - 1
        files.append(_mrc2(pick, [s32, s64, cnt, mx, mn]))
        for i, w in enumerate(pick):
            a = acc.get(w)
            row = [s32[i], s64[i], cnt[i], mx[i], mn[i]]
            acc[w] = row if a is None else [np.float32(a[0] + row[0]), a[1] + row[1], a[2] + row[2], max(a[3], row[3]),
                                            min(a[4], row[4])]
    want = {w: [a[0], np.float64(a[1]) / np.float64(a[2]), a[3], a[2], a[4]] for w, a in acc.items()}
    return files, want


def _bits(x) -> int:
    a = np.asarray(x)
    return int(a.view({4: np.uint32, 8: np.uint64}[a.dtype.itemsize]))


def _check_result(out: bytes, want: dict) -> None:
    cols = codec.decode_columns(out)
    off, blob = cols["key_off"], cols["key_blob"].tobytes()
    n = int(cols["hi"].size)
    keys = [blob[int(off[i]):int(off[i + 1])] for i in range(n)]
    assert all(a < b for a, b in zip(keys, keys[1:])), "keys not in strict bytewise order (or duplicated)"
    assert set(keys) == set(want)
    assert [c.dtype for c in cols["cols"]] == [np.float32, np.float64, np.float64, np.int64, np.int64]
    for i, k in enumerate(keys):
        got = [_bits(c[i]) for c in cols["cols"]]
        assert got == [_bits(v) for v in want[k]], (k, [c[i] for c in cols["cols"]], want[k])
    packed = [K.pack_key(k) for k in keys]
    assert cols["hi"].tolist() == [p[0] for p in packed] and cols["lo"].tolist() == [p[1] for p in packed]


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


@pytest.mark.parametrize("collide", [False, True], ids=["hash56", "hash2"])
@pytest.mark.parametrize("on_device", ["cpu", pytest.param("cuda", marks=pytest.mark.gpu)], indirect=True)
def test_typed_reduce_routes_match_python_fold(on_device, collide, monkeypatch):
    """Files as bytes, files read back from the store, and (GPU) files pulled
    inside the device: the same result as the dict fold, bit for bit.  With
    the long-key hash cut to 2 bits distinct long keys of different files
    meet on (hi, lo) and only their bytes in the pulled buffer tell them
    apart."""
    gpu = on_device.type == "cuda"
    try:
        if collide:
            K.set_long_hash_bits(2)
        files, want = _make_files()
        if collide:
            owners = {}
            for f, b in enumerate(files):
                c = codec.decode_columns(b)
                for h, l in zip(c["hi"].tolist(), c["lo"].tolist()):
                    if K.is_long(l):
                        owners.setdefault((h, l), set()).add(f)
            nlong = sum(1 for w in want if len(w) > K.PACK_MAX)
            assert len(owners) < nlong // 4 and any(len(s) > 1 for s in owners.values())
        _check_result(job_mod._device_reduce_cols(files, SPEC), want)
        st = hbm_store.store()
        descs = [x for _n, x in st.put_many([(f"red.P0.M{i}", b) for i, b in enumerate(files)])]
        assert job_mod._hbm_route_cols(descs, gpu) == ("pull" if gpu else "read")
        assert job_mod._hbm_route(descs, False, gpu) == "read"
        if gpu:
            calls = []
            real = hbm_store.HBMStore.read_many
            monkeypatch.setattr(hbm_store.HBMStore, "read_many", lambda self, d: calls.append(1) or real(self, d))
            before = st.stats["pulls"]
            _check_result(job_mod._device_reduce_cols_hbm(descs, SPEC), want)
            assert st.stats["pulls"] - before == NFILES and not calls
            monkeypatch.setattr(hbm_store.HBMStore, "read_many", real)
        blobs = st.read_many(descs)
        assert blobs == files
        _check_result(job_mod._device_reduce_cols(blobs, SPEC), want)
    finally:
        K.set_long_hash_bits(None)


# -- GPU: the same map both ways ------------------------------------------------------------------
def _csv() -> tuple[bytes, dict]:
    """A few thousand ``key,score`` rows over a few hundred keys (some longer
    than 15 bytes, up to 240) and their group-by: key -> scores."""
    rng = np.random.default_rng(21)
    letters = np.frombuffer(b"abcdefghijklmnopqrstuvwxyz", np.uint8)
    keys = sorted({rng.choice(letters, int(rng.integers(1, 16))).tobytes() for _ in range(260)})
    keys += [b"L%03dxyzw" % i + b"tail" * int(rng.integers(2, 14)) for i in range(40)]
    keys += [b"prefixAAprefixAA" + rng.choice(letters[:3], int(rng.integers(1, 30))).tobytes() for _ in range(30)]
    keys += [b"very-long-" + rng.choice(letters, 230).tobytes()]  # (256 bytes: the device's exact key order ends there)
    keys = sorted(set(keys))
    lines, groups = [], {}
    for _ in range(5000):
        k = keys[int(rng.integers(0, len(keys)))]
        v = int(rng.integers(0, 1 << 17)) / 8
        lines.append(k + b"," + (b"%.3f" % v))
        groups.setdefault(k, []).append(v)
    return b"\n".join(lines) + b"\n", groups


def _map_scores(key, value, emit):
    emit.csv(value, key=0, values=(1, 1, None), sep=",")  # (the fused CSV fold, as examples/ScoreStats)


def _map_mixed(key, value, emit):
    from lua_mapreduce_1_amd.ops import text as TX
    ks, kl, (score,) = TX.csv_rows(value, 0, (1,), ",")
    emit.spans(ks, kl, score.to(torch.float32), score, score, score.to(torch.float32), text=value)


# spec, device_mapfn, the physical columns' codes, the group-by's physical columns
MAPS = {
    "scores": (("f64:mean", "f64:max", "count"), _map_scores, [1, 0, 1],
               lambda v: [np.float64(sum(v)), np.int64(len(v)), np.float64(max(v))]),
    "f32_first": (("f32:sum", "f64:mean", "count", "f32:max"), _map_mixed, [2, 1, 0, 2],
                  lambda v: [np.float32(sum(v)), np.float64(sum(v)), np.int64(len(v)), np.float32(max(v))]),
}


class _Files:
    def __init__(self):
        self.items = []

    def store_many(self, items):
        self.items.extend(items)
        return True


def _map_job(text: torch.Tensor, nparts: int, files: _Files, mapfn):
    """A map job object with just what ``_run_generic_map`` uses: the
    coordinator's blob store is ``files``, the job table a stub."""
    class Cnn:
        dbname = "hbm_cols_device"

        def gridfs(self):
            return files

    class Jobs:
        def update(self, *a, **k):
            return {}

    j = job_mod.job.__new__(job_mod.job)
    j.cnn, j.jobs = Cnn(), Jobs()
    j.job_tbl = {"_id": 1, "value": text}
    j.task_tbl = {"iteration": 1, "extra": {"num_partitions": nparts, "table_capacity": 1 << 12}}
    j.storage, j.path, j.results_ns = "hbm", "/tmp/hbm_cols_device", "map_results"
    j.module = {"device_mapfn": mapfn}
    j.t, j.written = utils.time(), False
    return j


def _set_knob(monkeypatch, on: bool) -> None:
    monkeypatch.setattr(config, "TUNABLES", dataclasses.replace(config.TUNABLES, hbm_device_write=on))


def _run_map(text, nparts: int, which: str):
    spec, mapfn, _codes, _fold = MAPS[which]
    st = hbm_store.store()
    files = _Files()
    before = dict(st.stats)
    with dev.PLANE_LOCK:
        _map_job(text, nparts, files, mapfn)._run_generic_map(types.SimpleNamespace(device_partition=("fnv1", nparts)),
                                                              types.SimpleNamespace(device_reduce=spec), "cols")
    delta = {k: st.stats[k] - before[k] for k in before}
    descs = [(n, b) for n, b in files.items if hbm_store.is_descriptor(b)]
    index = sorted(n for n, b in files.items if not hbm_store.is_descriptor(b))
    assert descs and len(index) == len(descs) and delta["puts"] == len(descs)
    got = {n: (st.read_bytes(b), {k: v for k, v in hbm_store.HBMStore.parse(b).items() if k not in ("off", "c", "h")})
           for n, b in descs}
    return got, index, delta


@pytest.mark.gpu
@pytest.mark.parametrize("nparts", [1, 6, 256])
@pytest.mark.parametrize("which", list(MAPS))
def test_same_typed_fold_map_with_the_knob_on_and_off(gpu, monkeypatch, which, nparts):
    data, groups = _csv()
    text = torch.frombuffer(bytearray(data), dtype=torch.uint8).to(gpu)
    _spec, _mapfn, codes, fold = MAPS[which]
    got = {}
    for on in (True, False):
        _set_knob(monkeypatch, on)
        got[on], got[on, "index"], delta = _run_map(text, nparts, which)
        if on:
            # the device path ran (else the comparison below shows nothing)
            assert delta["dev_puts"] == delta["puts"] > 0 and delta["staged_bytes"] == 0
            assert delta["plan_bytes"] == 8 * (2 * nparts + 4)
        else:
            assert delta["dev_puts"] == 0 and delta["plan_bytes"] == 0
            assert delta["staged_bytes"] == delta["put_bytes"] > 0
    assert sorted(got[True]) == sorted(got[False]) and got[True, "index"] == got[False, "index"]
    for name in got[True]:
        assert got[True][name][0] == got[False][name][0], name  # the bytes
        assert got[True][name][1] == got[False][name][1], name  # host, pid, dev, len, rows, nb, mrc2
        d = got[True][name][1]
        assert (d["rows"], d["nb"]) == (-1, -1) and d["mrc2"]["codes"] == codes
        assert (d["mrc2"]["rows"], d["mrc2"]["nb"], d["mrc2"]["codes"]) == _head(got[True][name][0])
    # and they are the input's group-by, every key in one file
    seen = {}
    for name, (blob, _d) in got[True].items():
        c = codec.decode_columns(blob)
        kb = c["key_blob"].tobytes()
        keys = [kb[int(c["key_off"][i]):int(c["key_off"][i + 1])] for i in range(c["hi"].size)]
        assert all(a < b for a, b in zip(keys, keys[1:])), name
        for i, k in enumerate(keys):
            assert k not in seen
            seen[k] = [_bits(col[i]) for col in c["cols"]]
    assert seen == {k: [_bits(x) for x in fold(v)] for k, v in groups.items()}


@pytest.mark.gpu
def test_a_rejected_typed_plan_falls_back_to_the_same_files(gpu, monkeypatch):
    """The columns are sorted on the device when the plan is rejected (here:
    every plan): the host encoder then writes the same ``out`` — the files
    of the knob-off run, all of them staged, nothing reserved."""
    data, _groups = _csv()
    text = torch.frombuffer(bytearray(data), dtype=torch.uint8).to(gpu)
    got = {}
    for reject in (True, False):
        _set_knob(monkeypatch, reject)  # knob on with every plan rejected, then knob off
        seen, reserved = [], []
        real = dev.mrc2_file_plan
        real_reserve = hbm_store.HBMStore.reserve_many

        def plan(*a, **k):
            seen.append(real(*a, **k) is not None)
            return None

        monkeypatch.setattr(dev, "mrc2_file_plan", plan)
        monkeypatch.setattr(hbm_store.HBMStore, "reserve_many",
                            lambda self, *a, **k: reserved.append(1) or real_reserve(self, *a, **k))
        got[reject], _index, delta = _run_map(text, 6, "f32_first")
        monkeypatch.setattr(dev, "mrc2_file_plan", real)
        monkeypatch.setattr(hbm_store.HBMStore, "reserve_many", real_reserve)
        assert seen == ([True] if reject else [])  # the plan was a good one
        assert not reserved and delta["dev_puts"] == 0 and delta["plan_bytes"] == 0
        assert delta["staged_bytes"] == delta["put_bytes"] > 0
    assert got[True] and got[True] == got[False]


# -- GPU: a whole job ----------------------------------------------------------------------------
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


@pytest.mark.gpu
def test_scorestats_job_stages_nothing(gpu, cs, tmp_path, monkeypatch):
    """examples/ScoreStats over hbm storage with 2 GPU workers (threads: one
    store).  Knob on: every map file is written on the device and no reduce
    job reads one back to the host.  Knob off: the same result, staged."""
    from test_generic_plane import close_lists
    from test_generic_server_worker import SS, job as run
    st = hbm_store.store()
    calls = []
    real = hbm_store.HBMStore.read_many
    monkeypatch.setattr(hbm_store.HBMStore, "read_many",
                        lambda self, d: calls.append(_in_a_reduce_job()) or real(self, d))

    _set_knob(monkeypatch, True)
    before = dict(st.stats)
    got, exp, s = run(cs, tmp_path, "scores", SS, {}, "device", storage="hbm", db="cols_on")
    delta = {k: st.stats[k] - before[k] for k in before}
    assert close_lists(got, exp)
    assert s.last_stats["failed_map_jobs"] == 0 and s.last_stats["failed_red_jobs"] == 0
    assert delta["staged_bytes"] == 0
    assert delta["dev_puts"] > 0 and delta["dev_puts"] == delta["puts"]
    assert delta["plan_bytes"] > 0 and delta["pulls"] == delta["puts"]
    assert not any(calls)

    _set_knob(monkeypatch, False)
    del calls[:]
    before = dict(st.stats)
    got_off, exp, s = run(cs, tmp_path, "scores", SS, {}, "device", storage="hbm", db="cols_off")
    delta = {k: st.stats[k] - before[k] for k in before}
    assert close_lists(got_off, exp)
    assert s.last_stats["failed_map_jobs"] == 0 and s.last_stats["failed_red_jobs"] == 0
    assert delta["staged_bytes"] == delta["put_bytes"] > 0 and delta["dev_puts"] == 0
