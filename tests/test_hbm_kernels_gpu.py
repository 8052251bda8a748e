"""The two device kernels of ``hbm`` storage (csrc/hip/ipc.hip) against numpy,
and the store around them in one process on the GPU.

* ``mr_gather_copy`` vs numpy slicing: every head 0..15 of the head / 16-byte
  vector / tail split (also ``m < head``), the byte path of copies whose two
  sides differ mod 16, lengths round the copy chunk (several workgroups per
  copy), lists of 1, 2 and 40 copies (the binary search over ``chunk_start``),
  zero-length entries, ``n == 0``.  The destination is pre-filled; every
  byte outside the copies must keep the fill.
* ``mr_mrc1_decode`` vs ``codec.decode_columnar``: the row -> file search at
  the 255/256/257 block boundaries, one-row and zero-row files, the ``rep``
  offsets (checked by reading the keys back through them), nothing written
  outside the output columns.
* ``HBMStore``: put / read_bytes / read_many / pull_device round trip over
  several arena chunks.
"""
import struct

import numpy as np
import pytest
import torch

from lua_mapreduce_1_amd import ops
from lua_mapreduce_1_amd.ops import _hip
from lua_mapreduce_1_amd.ops import keys as K
from lua_mapreduce_1_amd.runtime import codec, hbm_store, job

pytestmark = pytest.mark.gpu

FILL = 0xA5      # the destination's fill; no source byte has this value
GAP = 32         # untouched bytes kept between (and round) the copies
ARENA = 4 << 20


@pytest.fixture(scope="module")
def arena(gpu):
    """(source bytes on the host, the same on the device, a destination
    tensor): both device tensors 16-byte aligned."""
    rng = np.random.default_rng(7)
    src = rng.integers(0, 255, ARENA, dtype=np.uint8)
    src[src >= FILL] += 1  # 0..255 without FILL: a copied byte never looks untouched
    assert not (src == FILL).any()
    s = torch.from_numpy(src).to(gpu)
    d = torch.empty(ARENA, dtype=torch.uint8, device=gpu)
    assert s.data_ptr() % 16 == 0 and d.data_ptr() % 16 == 0
    return src, s, d


def _chunk() -> int:
    return int(_hip.lib().mr_gather_copy_chunk())


def _place(specs):
    """[(src offset mod 16, dst offset mod 16, len)] -> [(src off, dst off,
    len)]: back to back on both sides, each at its offset mod 16, the
    destinations at least GAP bytes apart."""
    out, sc, dc = [], 0, GAP
    for smod, dmod, n in specs:
        so = (sc + 15) // 16 * 16 + smod
        do = (dc + 15) // 16 * 16 + dmod
        out.append((so, do, n))
        sc, dc = so + n, do + n + GAP
    return out


def _gather(arena, copies, gpu):
    """Run one launch over ``copies`` [(src off, dst off, len)] and compare
    the whole destination with numpy."""
    src, s, d = arena
    end = GAP
    for so, do, n in copies:  # in bounds, apart: checked on the host, before the launch
        assert 0 <= so and so + n <= ARENA
        assert end <= do and do + n + GAP <= ARENA
        end = do + n + GAP
    d.fill_(FILL)
    want = np.full(ARENA, FILL, np.uint8)
    for so, do, n in copies:
        want[do:do + n] = src[so:so + n]
    # the copy table, as HBMStore.pull_device builds it
    chunk = _chunk()
    lens = np.array([n for _, _, n in copies], np.uint64)
    nch = (lens + np.uint64(chunk - 1)) // np.uint64(chunk)
    start = np.zeros(len(copies), np.uint64)
    if len(copies) > 1:
        np.cumsum(nch[:-1], out=start[1:])
    tab = np.concatenate([np.uint64(s.data_ptr()) + np.array([c[0] for c in copies], np.uint64),
                          np.uint64(d.data_ptr()) + np.array([c[1] for c in copies], np.uint64), lens, start])
    t = torch.from_numpy(tab.view(np.int64)).to(gpu)
    _hip.call("mr_gather_copy", _hip.ptr(t), len(copies), int(nch.sum()), _hip.stream(gpu))
    got = d.cpu().numpy()
    bad = np.flatnonzero(got != want)
    assert bad.size == 0, f"{bad.size} wrong bytes, first at destination offset {int(bad[0])}; copies {copies[:8]}"


def _head_lens(head: int) -> list[int]:
    return sorted({n for n in (1, head - 1, head, head + 1, head + 15, head + 16, head + 17, 4113) if n > 0})


@pytest.mark.parametrize("head", range(16))
def test_gather_copy_same_offset_mod16(gpu, arena, head):
    """Both sides ``16 - head`` past a 16-byte boundary: ``head`` bytes, then
    vectors, then a byte tail; lengths below, at and past the head."""
    mod = (16 - head) % 16
    copies = _place([(mod, mod, n) for n in _head_lens(head)])
    _gather(arena, copies, gpu)
    for c in copies:  # each length alone too (one workgroup, one entry)
        _gather(arena, [c], gpu)


@pytest.mark.parametrize("smod,dmod", [(0, 1), (1, 0), (3, 11), (15, 8), (4, 12), (9, 10)])
def test_gather_copy_different_offsets_byte_path(gpu, arena, smod, dmod):
    copies = _place([(smod, dmod, n) for n in _head_lens((16 - smod) % 16)])
    _gather(arena, copies, gpu)


@pytest.mark.parametrize("smod,dmod", [(0, 0), (4, 4), (13, 13), (5, 10), (0, 8)])
def test_gather_copy_round_the_chunk_size(gpu, arena, smod, dmod):
    """Copies of G-1, G, G+1 and 3G+7 bytes: the last workgroup of a copy
    gets 0 < m <= G bytes, a later one starts ``k * G`` into both sides."""
    g = _chunk()
    copies = _place([(smod, dmod, n) for n in (g - 1, g, g + 1, 3 * g + 7)])
    _gather(arena, copies, gpu)
    _gather(arena, [copies[3]], gpu)


@pytest.mark.parametrize("ncopies", [1, 2, 40])
def test_gather_copy_lists_of_mixed_lengths(gpu, arena, ncopies):
    """The search over chunk_start: short and multi-chunk copies mixed, both
    paths in one launch."""
    g = _chunk()
    rng = np.random.default_rng(ncopies)
    specs = []
    for i in range(ncopies):
        n = int(rng.choice([1, 3, 16, 17, 100, 4113, 20_000]))
        if ncopies > 2 and i in (ncopies // 2, ncopies - 1):
            n = g + 19 if i == ncopies - 1 else 2 * g + 1
        elif i == 0:
            n = 65_537
        smod = int(rng.integers(0, 16))
        dmod = smod if rng.random() < 0.6 else int(rng.integers(0, 16))
        specs.append((smod, dmod, n))
    _gather(arena, _place(specs), gpu)


@pytest.mark.parametrize("lens", [[0, 500], [500, 0, 700], [500, 700, 0], [500, 0, 0, 700], [0, 0, 33, 0, 0],
                                  [0, 300_000, 0, 0, 5, 0], [0], [0, 0, 0]],
                         ids=["first", "middle", "last", "adjacent", "both_ends", "multi_chunk", "only", "all"])
def test_gather_copy_zero_length_entries(gpu, arena, lens):
    """Entries of no bytes own no chunk: chunk_start repeats, and the search
    must land on the entry that does."""
    for smod, dmod in ((4, 4), (2, 7)):
        _gather(arena, _place([(smod, dmod, n) for n in lens]), gpu)


def test_gather_copy_empty_list_is_a_noop(gpu, arena):
    src, s, d = arena
    d.fill_(FILL)
    t = torch.zeros(4, dtype=torch.int64, device=gpu)
    _hip.call("mr_gather_copy", _hip.ptr(t), 0, 0, _hip.stream(gpu))
    _hip.call("mr_gather_copy", None, 0, 0, _hip.stream(gpu))
    assert bool((d == FILL).all())


# -- mr_mrc1_decode -----------------------------------------------------------------
def _random_file(rng, n: int, packed: bool):
    """An MRC1 file of n rows and its columns.  ``packed``: hi/lo are the key
    words of the keys; else random bits over the whole u64 range."""
    lens = rng.integers(1, 41, n)
    lens[rng.random(n) < 0.02] = 300
    keys = [rng.integers(0, 256, int(ln), dtype=np.uint8).tobytes() for ln in lens]
    if packed:
        pk = [K.pack_key(k) for k in keys]
        hi = np.array([p[0] for p in pk], np.uint64).reshape(n)
        lo = np.array([p[1] for p in pk], np.uint64).reshape(n)
    else:
        hi = rng.integers(0, 2**64, n, dtype=np.uint64)
        lo = rng.integers(0, 2**64, n, dtype=np.uint64)
        hi[::3] |= np.uint64(1 << 63)
        lo[1::3] |= np.uint64(1 << 63)
    val = rng.integers(-2**63, 2**63 - 1, n, dtype=np.int64, endpoint=True)
    for i, v in enumerate((-2**63, 2**63 - 1, 0, -1)):
        val[i::11] = v
    key_off = np.zeros(n + 1, np.int64)
    np.cumsum(lens, out=key_off[1:])
    blob = np.frombuffer(b"".join(keys), np.uint8) if keys else np.zeros(0, np.uint8)
    return codec.encode_columnar(hi, lo, val, key_off, blob), keys


def _layout(files, gpu):
    lens = [len(b) for b in files]
    bases, total = job._aligned_bases(lens)
    host = np.full(max(total, 16), 0xEE, np.uint8)
    for o, b in zip(bases, files):
        host[o:o + len(b)] = np.frombuffer(b, np.uint8)
    heads = [struct.unpack_from("<qq", b, 4) for b in files]
    return torch.from_numpy(host).to(gpu), bases, [h[0] for h in heads], lens, [h[1] for h in heads]


def _expected(files, bases):
    cols = [codec.decode_columnar(b) for b in files]
    assert all(c["hi"].size == struct.unpack_from("<q", b, 4)[0] for c, b in zip(cols, files))
    rep = []
    for c, base in zip(cols, bases):
        n, ko = int(c["hi"].size), c["key_off"]
        rep += [K.make_rep(base + 20 + 8 * (4 * n + 1) + int(ko[k]), int(ko[k + 1] - ko[k])) for k in range(n)]
    cat = lambda name, dt: np.concatenate([c[name] for c in cols]).astype(dt)  # noqa: E731
    return cat("hi", np.uint64), cat("lo", np.uint64), cat("val", np.int64), np.array(rep, np.uint64)


@pytest.mark.parametrize("rows,packed", [([1], False), ([255, 256, 257], False), ([255, 256, 257], True),
                                         ([1000, 1, 1, 3000], False), ([0, 7, 0, 300, 0], False),
                                         ([0, 0, 256, 0, 0, 1], True), ([0], False)],
                         ids=lambda v: "-".join(map(str, v)) if isinstance(v, list) else ("keys" if v else "bits"))
def test_mrc1_decode_matches_host_decoder(gpu, rows, packed):
    rng = np.random.default_rng(sum(rows) + len(rows))
    made = [_random_file(rng, n, packed) for n in rows]
    files = [m[0] for m in made]
    keys = [k for m in made for k in m[1]]
    assert all(len(f) == 28 for f, n in zip(files, rows) if n == 0)
    buf, bases, hrows, lens, nbs = _layout(files, gpu)
    assert hrows == rows
    hi, lo, val, rep = job._decode_files(buf, bases, hrows, lens, nbs)
    w_hi, w_lo, w_val, w_rep = _expected(files, bases)
    n = sum(rows)
    assert hi.numel() == lo.numel() == val.numel() == rep.numel() == n
    assert np.array_equal(hi.cpu().numpy().view(np.uint64), w_hi)
    assert np.array_equal(lo.cpu().numpy().view(np.uint64), w_lo)
    assert np.array_equal(val.cpu().numpy(), w_val)
    got_rep = rep.cpu().numpy().view(np.uint64)
    assert np.array_equal(got_rep, w_rep)
    if n == 0:
        return
    # the keys read back through rep (all of rep checked above: inside buf).  Random hi/lo bits say
    # nothing about the key, so every row is marked long there and its bytes come from buf alone;
    # real key words go in as they are (packed keys from hi/lo, long ones from buf)
    lo_k = lo if packed else lo | 0xFF
    off, blob = ops.gather_key_bytes(hi, lo_k, rep, buf)
    off, blob = off.cpu().numpy(), blob.cpu().numpy().tobytes()
    assert [blob[int(off[i]):int(off[i + 1])] for i in range(n)] == keys


def test_mrc1_decode_writes_only_its_rows(gpu):
    """The kernel called directly, each output column inside a larger tensor
    of a sentinel: 64 elements before and after the n rows stay as they
    were (n = 513: a last block of one row; a zero-row file in the middle)."""
    rng = np.random.default_rng(3)
    rows = [255, 0, 258]
    files = [_random_file(rng, n, False)[0] for n in rows]
    buf, bases, hrows, lens, nbs = _layout(files, gpu)
    job._check_mrc1_layout(buf.numel(), bases, hrows, lens, nbs)
    n, pad, sent = sum(rows), 64, -0x0123456789ABCDEF
    rstart = np.zeros(len(rows) + 1, np.int64)
    np.cumsum(rows, out=rstart[1:])
    meta = torch.from_numpy(np.concatenate([np.asarray(bases, np.int64), rstart])).to(gpu)
    outs = [torch.full((n + 2 * pad,), sent, dtype=torch.int64, device=gpu) for _ in range(4)]
    views = [o[pad:pad + n] for o in outs]
    _hip.call("mr_mrc1_decode", _hip.ptr(buf), _hip.ptr(meta), len(rows), n, *[_hip.ptr(v) for v in views],
              _hip.stream(gpu))
    want = _expected(files, bases)
    for o, w in zip(outs, want):
        h = o.cpu().numpy()
        assert (h[:pad] == sent).all() and (h[pad + n:] == sent).all()
        assert np.array_equal(h[pad:pad + n].view(np.uint64), w.view(np.uint64))
    # no rows, no files: nothing is launched, nothing written
    _hip.call("mr_mrc1_decode", _hip.ptr(buf), _hip.ptr(meta), len(rows), 0, *[_hip.ptr(o) for o in outs],
              _hip.stream(gpu))
    _hip.call("mr_mrc1_decode", _hip.ptr(buf), _hip.ptr(meta), 0, 0, *[_hip.ptr(o) for o in outs], _hip.stream(gpu))
    assert all(int(o[0]) == sent for o in outs)


# -- HBMStore in one process ----------------------------------------------------------
def test_hbm_store_round_trip_over_several_chunks(gpu, monkeypatch):
    monkeypatch.setattr(hbm_store, "CHUNK", 1 << 20)
    rng = np.random.default_rng(9)
    raw = lambda n: rng.integers(0, 256, n, dtype=np.uint8).tobytes()  # noqa: E731
    col_big, _ = _random_file(rng, 4000, True)   # ~250 KB
    col_small, _ = _random_file(rng, 3, True)
    col_empty, _ = _random_file(rng, 0, True)
    rec_big = codec.encode_records([(f"key{i:07d}" * 3, [i, -i, i * i]) for i in range(7000)])  # ~300 KB
    rec_small = codec.encode_records([("a", [1])])
    items = [("raw1", raw(1)), ("col_big", col_big), ("raw15", raw(15)), ("rec_big", rec_big), ("raw16", raw(16)),
             ("col_empty", col_empty), ("raw17", raw(17)), ("raw300k", raw(300_001)), ("col_small", col_small),
             ("raw_huge", raw((3 << 19) + 5)), ("raw300k_b", raw(299_999)), ("rec_small", rec_small),
             ("col_big_b", col_big[:]), ("raw4", b"MRC1")]
    assert 200_000 < len(col_big) < 400_000 and 200_000 < len(rec_big) < 400_000
    st = hbm_store.HBMStore()
    try:
        descs = st.put_many(items[:9], gen=("db", 1)) + st.put_many(items[9:], gen=("db", 1))
        assert [n for n, _ in descs] == [n for n, _ in items]
        descs = [x for _n, x in descs]
        ds = [hbm_store.HBMStore.parse(x) for x in descs]
        data = [b for _n, b in items]
        for d, b in zip(ds, data):
            assert d["len"] == len(b) and d["off"] % 16 == 4 and d["dev"] == gpu.index and d["pid"] == st.pid
            if b[:4] == b"MRC1" and len(b) >= 20:
                assert (d["rows"], d["nb"]) == struct.unpack_from("<qq", b, 4)
            else:
                assert (d["rows"], d["nb"]) == (-1, -1)
        assert [d["rows"] for d in ds[:9]] == [-1, 4000, -1, -1, -1, 0, -1, -1, 3]
        # several chunks; files of one chunk do not overlap; the 1.5 MiB file has a chunk of its own
        by_chunk = {}
        for d in ds:
            by_chunk.setdefault(d["c"], []).append((d["off"], d["off"] + d["len"]))
        assert len(by_chunk) >= 3 and by_chunk[ds[9]["c"]] == [(4, 4 + len(data[9]))]
        for spans in by_chunk.values():
            spans.sort()
            assert all(a[1] <= b[0] for a, b in zip(spans, spans[1:]))
        assert st.stats["puts"] == len(items) and st.stats["put_bytes"] == sum(map(len, data))

        n = len(items)
        orders = [list(range(n)), list(rng.permutation(n)), [3, 3, 0, 9, 3, 0, 13, 9]]
        pulls = pull_bytes = 0
        for order in orders:
            ask, want = [descs[i] for i in order], [data[i] for i in order]
            assert [st.read_bytes(x) for x in ask] == want
            assert st.read_many(ask) == want
            buf, bases, got_ds = st.pull_device(ask, gpu)
            assert all(b % 16 == 4 for b in bases) and got_ds == [ds[i] for i in order]
            assert all(b0 + len(w) <= b1 for b0, w, b1 in zip(bases, want, bases[1:]))
            h = buf.cpu().numpy()
            assert [h[b:b + len(w)].tobytes() for b, w in zip(bases, want)] == want
            pulls += 2 * len(order)  # read_many pulls too
            pull_bytes += 2 * sum(map(len, want))
        assert st.stats["pulls"] == pulls and st.stats["pull_bytes"] == pull_bytes
        assert st.read_many([]) == []

        # the columnar files decode from the pulled buffer like from bytes
        cols = [i for i, d in enumerate(ds) if d["rows"] >= 0]
        buf, bases, got_ds = st.pull_device([descs[i] for i in cols], gpu)
        hi, lo, val, rep = job._decode_files(buf, bases, [d["rows"] for d in got_ds], [d["len"] for d in got_ds],
                                             [d["nb"] for d in got_ds])
        for got, w in zip((hi, lo, val, rep), _expected([data[i] for i in cols], bases)):
            assert np.array_equal(got.cpu().numpy().view(np.uint64), w.view(np.uint64))

        st.release()
        for x in (descs[0], descs[9]):
            with pytest.raises(RuntimeError, match=r"chunk \d+ of this process is gone"):
                st.read_bytes(x)
        with pytest.raises(RuntimeError, match=r"chunk \d+ of this process is gone"):
            st.pull_device(descs[:2], gpu)
    finally:
        st.release()
