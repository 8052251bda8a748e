"""``hbm`` storage, write side: a device fold map writes its partition files on
the device, straight into the worker's arena (``MR_HBM_DEVICE_WRITE``).

CPU: the owner protocol ``HBMStore.reserve_many`` / ``publish`` on the
``/dev/shm`` arena, and the pure decision whether the device may write
(``device.mrc1_file_plan``).

GPU: the same map through ``job._run_device_map_locked`` with the knob on and
off gives byte-identical files, and a whole word-count job with the knob on
stages no byte of its map files through the host.
"""
import dataclasses
import sys
import types

import numpy as np
import pytest
import torch

from lua_mapreduce_1_amd import utils
from lua_mapreduce_1_amd.runtime import codec, coordinator, device as dev, hbm_store, job as job_mod
from lua_mapreduce_1_amd.utils import config


# -- CPU: reserve / publish -------------------------------------------------------------
def _mrc1(rng, n: int) -> bytes:
    lens = rng.integers(1, 30, n)
    off = np.zeros(n + 1, np.int64)
    np.cumsum(lens, out=off[1:])
    return codec.encode_columnar(rng.integers(0, 2**64, n, dtype=np.uint64), rng.integers(0, 2**64, n, dtype=np.uint64),
                                 rng.integers(-2**63, 2**63 - 1, n, dtype=np.int64), off,
                                 rng.integers(0, 256, int(off[-1]), dtype=np.uint8))


@pytest.fixture
def shm_store():
    """A store of its own on the /dev/shm arena (also where a GPU is present)."""
    st = hbm_store.HBMStore()
    st._device = torch.device("cpu")
    yield st
    st.release()


def _header(b: bytes):
    return job_mod._mrc1_header(b)


def _write(places, files):
    for pl, b in zip(places, files):
        assert pl.ptr is None and pl.size == len(b)
        m = pl.mem
        m[:] = b
        del m  # (a live view would keep the chunk's mapping from closing)


def test_reserve_write_publish_read(shm_store):
    st = shm_store
    rng = np.random.default_rng(1)
    files = [_mrc1(rng, n) for n in (1, 300, 7)] + [b"not columnar"]
    names = [f"/x/map_results.P{i}.M1" for i in range(len(files))]
    sizes = [len(b) for b in files]
    rows = [_header(b)[0] for b in files]
    nbs = [_header(b)[1] for b in files]
    assert rows == [1, 300, 7, -1]
    places = st.reserve_many(sizes, gen=("db", 1))
    assert [pl.off % 16 for pl in places] == [hbm_store.ALIGN_MOD] * len(files)
    spans = sorted((pl.off, pl.off + pl.size) for pl in places)
    assert all(a[1] <= b[0] for a, b in zip(spans, spans[1:]))
    _write(places, files)
    descs = st.publish(names, places, sizes, rows, nbs, plan_bytes=8 * (2 * 4 + 4))
    assert [n for n, _ in descs] == names
    ds = [x for _n, x in descs]
    assert [st.read_bytes(x) for x in ds] == files
    assert st.read_many(ds) == files
    assert st.read_many(ds[::-1]) == files[::-1]
    # the descriptors are put_many's for the same bytes, except for the place
    put = st.put_many(list(zip(names, files)), gen=("db", 1))
    assert [n for n, _ in put] == names
    for (_n, a), (_m, b) in zip(descs, put):
        a, b = hbm_store.HBMStore.parse(a), hbm_store.HBMStore.parse(b)
        assert sorted(a) == sorted(b)
        assert {k: v for k, v in a.items() if k not in ("off", "c")} == \
               {k: v for k, v in b.items() if k not in ("off", "c")}
        assert (a["c"], a["off"]) != (b["c"], b["off"])
    assert [st.read_bytes(x) for _n, x in put] == files
    with pytest.raises(ValueError):
        st.publish(names[:2], places, sizes, rows, nbs)
    with pytest.raises(RuntimeError, match="reserved place"):
        st.publish(names[:1], places[:1], [sizes[0] + 1], rows[:1], nbs[:1])


def test_stats_count_staged_and_device_files_apart(shm_store):
    st = shm_store
    rng = np.random.default_rng(2)
    files = [_mrc1(rng, 5), _mrc1(rng, 9)]
    sizes = [len(b) for b in files]
    assert all(st.stats[k] == 0 for k in ("puts", "put_bytes", "staged_bytes", "dev_puts", "dev_put_bytes",
                                          "plan_bytes"))
    places = st.reserve_many(sizes, gen=("db", 1))
    assert st.stats["puts"] == 0 and st.stats["dev_puts"] == 0  # nothing is a file before publish
    _write(places, files)
    st.publish(["a", "b"], places, sizes, [5, 9], [_header(b)[1] for b in files], plan_bytes=48)
    assert (st.stats["puts"], st.stats["put_bytes"]) == (2, sum(sizes))
    assert (st.stats["dev_puts"], st.stats["dev_put_bytes"], st.stats["plan_bytes"]) == (2, sum(sizes), 48)
    assert st.stats["staged_bytes"] == 0
    st.put_many([("c", files[0])], gen=("db", 1))
    assert (st.stats["puts"], st.stats["put_bytes"]) == (3, sum(sizes) + sizes[0])
    assert st.stats["staged_bytes"] == sizes[0]
    assert (st.stats["dev_puts"], st.stats["dev_put_bytes"], st.stats["plan_bytes"]) == (2, sum(sizes), 48)


def test_a_new_generation_releases_the_arena(shm_store):
    st = shm_store
    rng = np.random.default_rng(3)
    f1, f2 = _mrc1(rng, 4), _mrc1(rng, 6)
    p1 = st.reserve_many([len(f1)], gen=("db", 1))
    _write(p1, [f1])
    (_n, d1), = st.publish(["one"], p1, [len(f1)], [4], [_header(f1)[1]])
    assert st.read_bytes(d1) == f1
    p_same = st.reserve_many([len(f2)], gen=("db", 1))  # same generation: the arena stays
    assert st.read_bytes(d1) == f1 and p_same[0].chunk is p1[0].chunk
    p2 = st.reserve_many([len(f2)], gen=("db", 2))
    with pytest.raises(RuntimeError, match=r"chunk \d+ of this process is gone"):
        st.read_bytes(d1)
    with pytest.raises(RuntimeError, match="released"):
        st.publish(["late"], p_same, [len(f2)], [6], [_header(f2)[1]])
    _write(p2, [f2])
    (_n, d2), = st.publish(["two"], p2, [len(f2)], [6], [_header(f2)[1]])
    assert st.read_bytes(d2) == f2


def test_a_file_over_the_chunk_size_gets_its_own_chunk(shm_store, monkeypatch):
    monkeypatch.setattr(hbm_store, "CHUNK", 1 << 20)
    st = shm_store
    big = (3 << 19) + 5
    places = st.reserve_many([1000, big, 2000, 600_000, 600_000], gen=("db", 1))
    small, huge, after = places[0], places[1], places[2]
    assert huge.chunk is not small.chunk and huge.off == hbm_store.ALIGN_MOD and huge.chunk.size >= big + 4
    assert after.chunk is not huge.chunk or after.off >= huge.off + big
    assert places[4].chunk is not places[3].chunk  # two 600 kB files do not share a 1 MiB chunk
    for pl in places:
        assert pl.off % 16 == hbm_store.ALIGN_MOD and pl.off + pl.size <= pl.chunk.size
    data = np.random.default_rng(4).integers(0, 256, big, dtype=np.uint8).tobytes()
    _write([huge], [data])
    (_n, d), = st.publish(["huge"], [huge], [big], [-1], [-1])
    assert st.read_bytes(d) == data


def test_device_write_decision():
    """``mrc1_file_plan``: None for every flag bit of the tail, for a set sort
    error word, for key bytes past the blob capacity and for counts that do
    not add up; else the non-empty partitions' files."""
    rows = np.array([3, 0, 2, 0], np.int64)
    nbs = np.array([10, 0, 7, 0], np.int64)

    def plan(bad=0, err=0, total=17, nrows=5):
        return np.concatenate([rows, nbs, [bad, err, total, nrows]]).astype(np.int64)

    got = dev.mrc1_file_plan(plan(), 5, 4, 17)
    assert got is not None
    parts, starts, r, b, sizes = got
    assert (parts.tolist(), starts.tolist(), r.tolist(), b.tolist()) == ([0, 2], [0, 3], [3, 2], [10, 7])
    assert sizes.tolist() == [28 + 32 * 3 + 10, 28 + 32 * 2 + 7]
    assert dev.mrc1_file_plan(plan(), 5, 4, 1 << 30) is not None
    for bit in range(5):
        assert dev.mrc1_file_plan(plan(bad=1 << bit), 5, 4, 17) is None
    assert dev.mrc1_file_plan(plan(bad=3), 5, 4, 17) is None
    for err in (1, 4, 0x7FFFFFFF):
        assert dev.mrc1_file_plan(plan(err=err), 5, 4, 17) is None
    assert dev.mrc1_file_plan(plan(), 5, 4, 16) is None          # off[n] > blob_cap
    assert dev.mrc1_file_plan(plan(total=18), 5, 4, 17) is None  # ... as the device reports it
    assert dev.mrc1_file_plan(plan(nrows=6), 5, 4, 17) is None   # the counts are not the n rows
    assert dev.mrc1_file_plan(plan(), 6, 4, 17) is None


def test_knob_is_on_by_default_and_reads_its_variable():
    assert config.Tunables.from_env({}).hbm_device_write is True
    assert config.Tunables.from_env({"MR_HBM_DEVICE_WRITE": "0"}).hbm_device_write is False


# -- GPU: the same map both ways --------------------------------------------------------------
def _corpus() -> bytes:
    """A few thousand words of at most 15 bytes (packed keys) and 20 longer
    ones (keys kept by their bytes) whose first 8 bytes differ, so no two long
    keys tie on their prefix: the fused tail raises no flag."""
    rng = np.random.default_rng(11)
    letters = np.frombuffer(b"abcdefghijklmnopqrstuvwxyz", np.uint8)
    vocab = [rng.choice(letters, int(rng.integers(1, 16))).tobytes() for _ in range(1500)]
    long_words = [b"L%03dxyzw" % i + b"tail" * int(rng.integers(3, 14)) for i in range(20)]
    assert len({w[:8] for w in long_words}) == 20 and all(16 < len(w) <= 64 for w in long_words)
    words = [vocab[int(i)] for i in rng.integers(0, len(vocab), 4000)]
    for i, w in enumerate(long_words):
        words.insert(int(rng.integers(0, len(words))), w)
        words.insert(int(rng.integers(0, len(words))), w if i % 2 else vocab[i])
    return b" ".join(words) + b"\n"


class _Files:
    def __init__(self):
        self.items = []

    def store_many(self, items):
        self.items.extend(items)
        return True


def _map_job(text: torch.Tensor, nparts: int, files: _Files):
    """A map job object with just what ``_run_device_map_locked`` uses: the
    coordinator's blob store is ``files``, the job table a stub."""
    class Cnn:
        dbname = "hbm_device_write"

        def gridfs(self):
            return files

    class Jobs:
        def update(self, *a, **k):
            return {}

    j = job_mod.job.__new__(job_mod.job)
    j.cnn, j.jobs = Cnn(), Jobs()
    j.job_tbl = {"_id": 1, "value": text}
    j.task_tbl = {"iteration": 1, "extra": {"num_partitions": nparts, "table_capacity": 1 << 16}}
    j.storage, j.path, j.results_ns = "hbm", "/tmp/hbm_device_write", "map_results"
    j.module = {"device_mapfn": lambda key, value, emit: emit.words(value)}
    j.t, j.written = utils.time(), False
    return j


def _set_knob(monkeypatch, on: bool) -> None:
    monkeypatch.setattr(config, "TUNABLES", dataclasses.replace(config.TUNABLES, hbm_device_write=on))


@pytest.mark.gpu
@pytest.mark.parametrize("nparts", [1, 10, 256])
def test_same_map_with_the_knob_on_and_off(gpu, monkeypatch, nparts):
    text = torch.frombuffer(bytearray(_corpus()), dtype=torch.uint8).to(gpu)
    st = hbm_store.store()
    got = {}
    for on in (True, False):
        _set_knob(monkeypatch, on)
        files = _Files()
        before = dict(st.stats)
        with dev.PLANE_LOCK:
            _map_job(text, nparts, files)._run_device_map_locked(
                types.SimpleNamespace(device_partition=("fnv1", nparts)), types.SimpleNamespace(device_reduce="sum"))
        delta = {k: st.stats[k] - before[k] for k in before}
        descs = [(n, b) for n, b in files.items if hbm_store.is_descriptor(b)]
        index = [n for n, b in files.items if not hbm_store.is_descriptor(b)]
        assert descs and len(index) == len(descs) and delta["puts"] == len(descs)
        if on:
            # the device path ran (else the comparison below shows nothing)
            assert delta["dev_puts"] == len(descs) > 0 and delta["staged_bytes"] == 0
            assert delta["plan_bytes"] == 8 * (2 * nparts + 4)
        else:
            assert delta["dev_puts"] == 0 and delta["staged_bytes"] == delta["put_bytes"] > 0
        got[on] = {n: (st.read_bytes(b), {k: v for k, v in hbm_store.HBMStore.parse(b).items()
                                          if k not in ("off", "c", "h")}) for n, b in descs}
        got[on, "index"] = sorted(index)
    assert sorted(got[True]) == sorted(got[False]) and got[True, "index"] == got[False, "index"]
    for name in got[True]:
        assert got[True][name][0] == got[False][name][0], name  # the bytes
        assert got[True][name][1] == got[False][name][1], name  # host, pid, dev, len, rows, nb
    # and they are the corpus' counts
    counts = {}
    for name, (blob, _d) in got[True].items():
        c = codec.decode_columnar(blob)
        kb = c["key_blob"].tobytes()
        for i in range(c["hi"].size):
            k = kb[int(c["key_off"][i]):int(c["key_off"][i + 1])]
            assert k not in counts
            counts[k] = int(c["val"][i])
    want = {}
    for w in _corpus().split():
        want[w] = want.get(w, 0) + 1
    assert counts == want


@pytest.mark.gpu
def test_a_rejected_plan_falls_back_to_the_same_files(gpu, monkeypatch):
    """The device tail has already run on the table when the plan is
    rejected (here: every plan, as if the tail had raised a flag).
    ``finalize_table`` then runs the whole tail on the same table: the files
    are those of the knob-off run, all of them staged, none reserved."""
    nparts = 10
    text = torch.frombuffer(bytearray(_corpus()), dtype=torch.uint8).to(gpu)
    st = hbm_store.store()
    got = {}
    for reject in (True, False):
        _set_knob(monkeypatch, reject)  # knob on with every plan rejected, then knob off
        seen = []
        real = dev.mrc1_file_plan

        def plan(*a, **k):
            seen.append(real(*a, **k) is not None)
            return None

        monkeypatch.setattr(dev, "mrc1_file_plan", plan)
        files = _Files()
        before = dict(st.stats)
        with dev.PLANE_LOCK:
            _map_job(text, nparts, files)._run_device_map_locked(
                types.SimpleNamespace(device_partition=("fnv1", nparts)), types.SimpleNamespace(device_reduce="sum"))
        monkeypatch.setattr(dev, "mrc1_file_plan", real)
        delta = {k: st.stats[k] - before[k] for k in before}
        assert seen == ([True] if reject else [])  # the device tail ran and its plan was a good one
        assert delta["dev_puts"] == 0 and delta["plan_bytes"] == 0
        assert delta["staged_bytes"] == delta["put_bytes"] > 0
        got[reject] = {n: st.read_bytes(b) for n, b in files.items if hbm_store.is_descriptor(b)}
    assert got[True] and got[True] == got[False]


# -- GPU: a whole job -------------------------------------------------------------------------
@pytest.fixture(scope="module")
def cs():
    return coordinator.start_local()


def _in_a_map_job() -> bool:
    f = sys._getframe(1)
    while f is not None:
        if f.f_code.co_name == "_run_device_map_locked":
            return True
        f = f.f_back
    return False


@pytest.mark.gpu
def test_wordcount_job_stages_nothing(gpu, cs, monkeypatch):
    """Word count over hbm storage with 2 GPU workers (threads: one store).
    Knob on: every map file is written on the device — no staged byte, no
    ``finalize_host`` (the tail's download half) inside a map job.  Knob off:
    the same job stages its files and prints the same output.  (The corpus
    is the scenario's own: none of its map jobs falls back.)"""
    from test_e2e_wordcount import SCENARIOS, naive_output, run_job
    st = hbm_store.store()
    calls = []
    real = dev.finalize_host

    def spy(*a, **k):
        calls.append(_in_a_map_job())
        return real(*a, **k)

    monkeypatch.setattr(dev, "finalize_host", spy)
    p = dict(SCENARIOS["combiner_aci"], storage="hbm", device="auto")

    _set_knob(monkeypatch, True)
    before = dict(st.stats)
    got, s = run_job(cs, "hbm_dw_on", p, nworkers=2)
    delta = {k: st.stats[k] - before[k] for k in before}
    assert got == naive_output()
    assert s.last_stats["failed_map_jobs"] == 0 and s.last_stats["failed_red_jobs"] == 0
    assert delta["staged_bytes"] == 0
    assert delta["dev_puts"] > 0 and delta["dev_puts"] == delta["puts"]
    assert delta["plan_bytes"] > 0
    assert not any(calls)

    _set_knob(monkeypatch, False)
    del calls[:]
    before = dict(st.stats)
    got_off, s = run_job(cs, "hbm_dw_off", p, nworkers=2)
    delta = {k: st.stats[k] - before[k] for k in before}
    assert got_off == got
    assert s.last_stats["failed_map_jobs"] == 0 and s.last_stats["failed_red_jobs"] == 0
    assert delta["staged_bytes"] > 0 and delta["dev_puts"] == 0
    assert any(calls)
