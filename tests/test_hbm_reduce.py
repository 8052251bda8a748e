"""The reduce side of ``hbm`` storage against a Python fold, and the host-side
guards in front of its kernels.

* ``job._device_reduce`` (files as bytes), ``HBMStore.read_many`` ->
  ``job._device_reduce`` (CPU arena) and ``HBMStore.put_many`` ->
  ``job._device_reduce_hbm`` (GPU arena: gather copy + MRC1 decode,
  csrc/hip/ipc.hip) fold five overlapping map files of one partition; the
  result must be a dict fold of every input row, keys in strict bytewise
  order.  Once more with the long-key hash cut to 2 bits, so that distinct
  long keys of *different files* meet on (hi, lo) and only their bytes in
  the pulled buffer tell them apart.
* ``job._decode_files`` refuses, before it allocates or launches anything, a
  negative row count (a host map's MRK1 file: ``rows = -1`` in its
  descriptor) and a header that does not account for the file's length;
  ``job._hbm_route`` sends only all-columnar file sets down the pulled path.
* Nodes that mix CPU and GPU workers: a ``/dev/shm`` descriptor in a GPU
  reader, a GPU descriptor in a process without a GPU.
"""
import json
import os

import numpy as np
import pytest
import torch

from lua_mapreduce_1_amd.ops import keys as K
from lua_mapreduce_1_amd.runtime import codec, hbm_store, job
from lua_mapreduce_1_amd.runtime import device as devmod

NFILES = 5
I64_MIN, I64_MAX = -2**63, 2**63 - 1


def _words() -> list[bytes]:
    """~2000 distinct keys: packed ones of every length 1..15, long ones that
    share 8-byte and 16-byte prefixes over a tiny alphabet (near-duplicates,
    like test_exactness.colliding_text), a few very long, a few with bytes
    >= 0x80 (not 7-bit: the sort's exact path)."""
    rng = np.random.default_rng(11)
    seen: set = set()

    def add(w):
        seen.add(bytes(w))

    for n in range(1, 16):
        for _ in range(30):
            add(rng.integers(97, 123, n).astype(np.uint8).tobytes())
    for w in (b"a", b"prefixAA", b"prefixAAbcd", b"prefixAAprefixA", b"prefixAAprefixAA", b"\xff",
              b"\xc3\xa9t\xc3\xa9"):
        add(w)
    prefixes = [b"prefixAA", b"prefixAB", b"zzzzzzzz", b"prefixAAprefixAA", b"prefixAAprefixAB",
                b"caf\xc3\xa9\xe2\x82\xac-"]
    while len(seen) < 2000:
        p = prefixes[int(rng.integers(0, len(prefixes)))]
        n = int(rng.integers(8, 40)) if rng.random() < 0.98 else int(rng.integers(200, 400))
        add(p + rng.integers(97, 100, n).astype(np.uint8).tobytes())
    return sorted(seen)


WORDS = _words()


def _make_files(op: str):
    """(files, want): five MRC1 map outputs of one partition, built in pure
    Python (pack_key under the current hash mask, keys sorted bytewise), and
    the dict fold of all their rows."""
    rng = np.random.default_rng({"sum": 1, "min": 2, "max": 3, "count": 4}[op])
    fold = {"sum": lambda a, b: a + b, "count": lambda a, b: a + b, "min": min, "max": max}[op]
    files, want = [], {}
    for f in range(NFILES):
        pick = [w for w in WORDS if rng.random() < 0.55]  # overlapping key sets, each sorted
        if op in ("min", "max"):
            vals = rng.integers(I64_MIN, I64_MAX, len(pick), dtype=np.int64, endpoint=True)
            vals[::97] = I64_MIN
            vals[1::89] = I64_MAX
        else:  # sums of five stay far from the int64 range
            vals = rng.integers(-2**40, 2**40, len(pick), dtype=np.int64)
        vals[2::53] = 0
        vals[3::59] = -1
        packed = [K.pack_key(w) for w in pick]
        hi = np.array([p[0] for p in packed], np.uint64)
        lo = np.array([p[1] for p in packed], np.uint64)
        key_off = np.zeros(len(pick) + 1, np.int64)
        np.cumsum([len(w) for w in pick], out=key_off[1:])
        blob = np.frombuffer(b"".join(pick), np.uint8)
        files.append(codec.encode_columnar(hi, lo, vals, key_off, blob))
        for w, v in zip(pick, vals.tolist()):
            want[w] = fold(want[w], v) if w in want else v
    return files, want


def _check_result(out: bytes, want: dict) -> None:
    cols = codec.decode_columnar(out)
    off, blob = cols["key_off"], cols["key_blob"].tobytes()
    keys = [blob[int(off[i]):int(off[i + 1])] for i in range(cols["val"].size)]
    assert all(a < b for a, b in zip(keys, keys[1:])), "keys not in strict bytewise order (or duplicated)"
    assert dict(zip(keys, cols["val"].tolist())) == want
    # the key words are those of the bytes
    packed = [K.pack_key(k) for k in keys]
    assert cols["hi"].tolist() == [p[0] for p in packed]
    assert cols["lo"].tolist() == [p[1] for p in packed]


@pytest.fixture
def on_device(request, monkeypatch, tmp_path):
    """Run the reduce functions on the given device ("cpu": also on a machine
    with a GPU) with a fresh process store whose CPU arena lives in tmp_path."""
    name = request.param
    if name == "cuda":
        request.getfixturevalue("gpu")
        d = torch.device("cuda", 0)
    else:
        d = torch.device("cpu")
    monkeypatch.setattr(devmod, "default_device", lambda: d)
    monkeypatch.setenv("MR_HBM_SHM_DIR", str(tmp_path))
    st = hbm_store.HBMStore()
    monkeypatch.setattr(hbm_store, "_STORE", st)
    try:
        yield d
    finally:
        st.release()


DEVICES = ["cpu", pytest.param("cuda", marks=pytest.mark.gpu)]


@pytest.mark.parametrize("collide", [False, True], ids=["hash56", "hash2"])
@pytest.mark.parametrize("op", ["sum", "min", "max", "count"])
@pytest.mark.parametrize("on_device", DEVICES, indirect=True)
def test_reduce_routes_match_python_fold(on_device, op, collide):
    try:
        if collide:
            K.set_long_hash_bits(2)
        files, want = _make_files(op)
        if collide:  # distinct long keys of different files do share (hi, lo)
            first = {}
            for f, b in enumerate(files):
                c = codec.decode_columnar(b)
                for h, l in zip(c["hi"].tolist(), c["lo"].tolist()):
                    if K.is_long(l):
                        first.setdefault((h, l), set()).add(f)
            nlong = sum(1 for w in want if len(w) > K.PACK_MAX)
            assert len(first) < nlong // 4 and any(len(s) > 1 for s in first.values())
        _check_result(job._device_reduce(files, op), want)
        st = hbm_store.store()
        descs = [x for _n, x in st.put_many([(f"red.P0.M{i}", b) for i, b in enumerate(files)])]
        assert job._hbm_route(descs, True, on_device.type == "cuda") == ("pull" if on_device.type == "cuda" else "read")
        if on_device.type == "cuda":
            _check_result(job._device_reduce_hbm(descs, op), want)
            assert st.stats["pulls"] == NFILES
        blobs = st.read_many(descs)
        assert blobs == files
        _check_result(job._device_reduce(blobs, op), want)
    finally:
        K.set_long_hash_bits(None)


# -- guards ---------------------------------------------------------------------
def _small_file(n: int, seed: int = 0) -> bytes:
    rng = np.random.default_rng(seed)
    words = sorted({rng.integers(97, 123, int(rng.integers(1, 30))).astype(np.uint8).tobytes()
                    for _ in range(2 * n)})[:n]
    packed = [K.pack_key(w) for w in words]
    key_off = np.zeros(n + 1, np.int64)
    np.cumsum([len(w) for w in words], out=key_off[1:])
    return codec.encode_columnar(np.array([p[0] for p in packed], np.uint64),
                                 np.array([p[1] for p in packed], np.uint64),
                                 rng.integers(-9, 9, n, dtype=np.int64), key_off,
                                 np.frombuffer(b"".join(words), np.uint8))


@pytest.fixture
def no_launch(monkeypatch):
    """Any allocation or native call after the guard fails the test."""
    from lua_mapreduce_1_amd.ops import _hip

    def boom(*a, **k):
        raise AssertionError("reached an allocation or a launch")
    class NoTorch:
        def __getattr__(self, name):
            boom()
    monkeypatch.setattr(_hip, "call", boom)
    monkeypatch.setattr(_hip, "lib", boom)
    monkeypatch.setattr(job, "torch", NoTorch())  # (the module's own name for torch: the tests' stays)


@pytest.fixture
def cpu_store(monkeypatch, tmp_path):
    monkeypatch.setattr(devmod, "default_device", lambda: torch.device("cpu"))
    monkeypatch.setenv("MR_HBM_SHM_DIR", str(tmp_path))
    st = hbm_store.HBMStore()
    try:
        yield st
    finally:
        st.release()


def _layout(files):
    lens = [len(b) for b in files]
    bases, total = job._aligned_bases(lens)
    buf = np.zeros(total, np.uint8)
    for o, b in zip(bases, files):
        buf[o:o + len(b)] = np.frombuffer(b, np.uint8)
    heads = [job._mrc1_header(b) for b in files]
    return torch.from_numpy(buf), bases, [h[0] for h in heads], lens, [h[1] for h in heads]


def test_decode_files_refuses_negative_rows(cpu_store, no_launch):
    """What the parent commit handed the kernel: the descriptors of a host
    map's record files carry rows = -1, summed to a negative (as u64: huge)
    row count."""
    recs = [codec.encode_records([("a", [1]), ("b", [2, 3])]), codec.encode_records([("c", [4])])]
    ds = [hbm_store.HBMStore.parse(x) for _n, x in cpu_store.put_many([("m0", recs[0]), ("m1", recs[1])])]
    rows, lens, nbs = [d["rows"] for d in ds], [d["len"] for d in ds], [d["nb"] for d in ds]
    assert rows == [-1, -1]
    bases, total = job._aligned_bases(lens)
    buf = torch.zeros(total, dtype=torch.uint8)
    with pytest.raises(ValueError, match="row count -1"):
        job._decode_files(buf, bases, rows, lens, nbs)
    # one bad file among good ones
    buf, bases, rows, lens, nbs = _layout([_small_file(5, 1), _small_file(7, 2), _small_file(3, 3)])
    with pytest.raises(ValueError, match="file 1 has row count -1"):
        job._decode_files(buf, bases, [rows[0], -1, rows[2]], lens, nbs)
    with pytest.raises(ValueError, match="row count"):
        job._decode_files(buf, bases, [rows[0], rows[1], -2**63], lens, nbs)


@pytest.mark.parametrize("what", ["truncated", "padded", "rows+1", "rows-1", "nb+1", "nb-8", "huge_rows", "outside",
                                  "misaligned"])
def test_decode_files_refuses_inconsistent_header(no_launch, what):
    """20 + 8 * (4 n + 1) + nb must be the file's length, and the file must
    lie in the buffer where its 8-byte columns are aligned."""
    files = [_small_file(5, 1), _small_file(40, 2), _small_file(3, 3)]
    buf, bases, rows, lens, nbs = _layout(files)
    assert all(20 + 8 * (4 * n + 1) + nb == ln for n, nb, ln in zip(rows, nbs, lens))
    if what == "truncated":
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
        rows[1] = 2**61 + rows[1]  # 32 n wraps to the same value in 64-bit arithmetic
    elif what == "outside":
        buf = buf[:bases[2] + lens[2] - 1].clone()
    elif what == "misaligned":
        bases[1] += 4
    with pytest.raises(ValueError, match="MRC1 decode: file"):
        job._decode_files(buf, bases, rows, lens, nbs)


def test_device_reduce_header_of_a_blob():
    b = _small_file(9, 4)
    assert job._mrc1_header(b) == (9, len(b) - 20 - 8 * 37)
    assert job._mrc1_header(codec.encode_records([("a", [1])])) == (-1, -1)
    assert job._mrc1_header(b"MRC1") == (-1, -1) and job._mrc1_header(b"") == (-1, -1)
    empty = codec.encode_columnar(np.zeros(0, np.uint64), np.zeros(0, np.uint64), np.zeros(0, np.int64),
                                  np.zeros(1, np.int64), np.zeros(0, np.uint8))
    assert len(empty) == 28 and job._mrc1_header(empty) == (0, 0)


def test_hbm_route_pulls_only_columnar_files(cpu_store):
    col = [(f"c{i}", _small_file(4 + i, i)) for i in range(3)]
    col.append(("c_empty", codec.encode_columnar(np.zeros(0, np.uint64), np.zeros(0, np.uint64), np.zeros(0, np.int64),
                                                 np.zeros(1, np.int64), np.zeros(0, np.uint8))))
    rec = [(f"r{i}", codec.encode_records([(f"k{i}", [i])])) for i in range(2)]
    dcol = [x for _n, x in cpu_store.put_many(col)]
    drec = [x for _n, x in cpu_store.put_many(rec)]
    assert [hbm_store.HBMStore.parse(x)["rows"] for x in dcol] == [4, 5, 6, 0]
    assert [hbm_store.HBMStore.parse(x)["rows"] for x in drec] == [-1, -1]
    assert job._hbm_route(dcol, True, True) == "pull"
    assert job._hbm_route(drec, True, True) == "read"
    for mix in (dcol + drec, drec + dcol, dcol[:1] + drec[:1] + dcol[1:], [drec[0]], dcol + drec[-1:]):
        assert job._hbm_route(mix, True, True) == "read"
    assert job._hbm_route(dcol, False, True) == "read"  # a typed (MRC2) fold decodes on the host
    assert job._hbm_route(dcol, True, False) == "read"  # no GPU
    legacy = hbm_store.MAGIC + json.dumps({k: v for k, v in hbm_store.HBMStore.parse(dcol[0]).items()
                                           if k != "rows"}).encode()
    assert job._hbm_route([legacy], True, True) == "read"  # no row count: not known to be columnar


# -- nodes that mix CPU and GPU workers -------------------------------------------
def _foreign(st, path, off: int, n: int, dev: int) -> bytes:
    """The descriptor another worker process of this host would publish."""
    d = {"host": st.host, "pid": os.getpid() + 1, "dev": dev, "c": 0, "h": str(path).encode().hex(), "off": off,
         "len": n, "rows": -1, "nb": -1}
    return hbm_store.MAGIC + json.dumps(d, separators=(",", ":")).encode()


def _shm_file(tmp_path, n: int, off: int = 20):
    data = np.random.default_rng(n).integers(0, 256, off + n + 9, dtype=np.uint8).tobytes()
    p = tmp_path / f"peer_chunk_{n}"
    p.write_bytes(data)
    return p, data[off:off + n]


def test_cpu_reader_reads_cpu_peer(cpu_store, tmp_path):
    p, want = _shm_file(tmp_path, 1000)
    desc = _foreign(cpu_store, p, 20, 1000, -1)
    own = cpu_store.put_many([("mine", b"0123456789")])[0][1]
    assert cpu_store.read_bytes(desc) == want
    assert cpu_store.read_many([own, desc, desc]) == [b"0123456789", want, want]
    gone = _foreign(cpu_store, tmp_path / "no_such_chunk", 0, 4, -1)
    with pytest.raises(RuntimeError, match="is gone"):
        cpu_store.read_bytes(gone)


@pytest.mark.skipif(torch.cuda.is_available(), reason="a process with a GPU opens the handle")
def test_cpu_reader_refuses_gpu_descriptor(cpu_store, tmp_path):
    desc = _foreign(cpu_store, "00" * 64, 4, 100, 0)
    for read in (cpu_store.read_bytes, lambda x: cpu_store.read_many([x])):
        with pytest.raises(RuntimeError, match=r"memory of GPU 0 \(owner pid \d+\).*no GPU"):
            read(desc)


@pytest.mark.gpu
def test_gpu_reader_stages_cpu_peer(gpu, monkeypatch, tmp_path):
    """A GPU reducer pulls a CPU worker's /dev/shm file together with a file
    of a GPU arena (on the parent commit: TypeError, mmap + int)."""
    monkeypatch.setattr(devmod, "default_device", lambda: gpu)
    st = hbm_store.HBMStore()
    try:
        p1, w1 = _shm_file(tmp_path, 5000)
        p2, w2 = _shm_file(tmp_path, 17, off=3)
        mine = np.random.default_rng(5).integers(0, 256, 3001, dtype=np.uint8).tobytes()
        own = st.put_many([("mine", mine)])[0][1]
        descs = [_foreign(st, p1, 20, 5000, -1), own, _foreign(st, p2, 3, 17, -1), own, _foreign(st, p1, 20, 5000, -1)]
        want = [w1, mine, w2, mine, w1]
        buf, bases, ds = st.pull_device(descs, gpu)
        h = buf.cpu().numpy()
        assert all(b % 16 == 4 for b in bases)
        assert [h[b:b + d["len"]].tobytes() for b, d in zip(bases, ds)] == want
        assert st.read_many(descs) == want
        assert st.read_bytes(descs[2]) == w2
    finally:
        st.release()
