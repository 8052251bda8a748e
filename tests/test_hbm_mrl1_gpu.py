"""The MRL1 device codec of ``hbm`` storage (csrc/hip/ipc.hip) against the
host codec (``codec.encode_lists`` / ``codec.decode_lists``).

* ``mr_mrl1_plan``: rows, key bytes and values of every partition and the
  three totals against numpy, also for counts that sum past the n rows
  (clamped by the kernel, then refused by ``device.mrl1_file_plan``).
* ``mr_mrl1_encode``: every non-empty partition's file of a sorted table in
  ONE launch, into a destination filled with a sentinel: the whole
  destination is compared, so every byte outside the files must keep the
  fill.  Files of 1, 2, 255, 256 and 257 rows, 1, 6 and 256 partitions; files
  without a value, with an odd and an even value count (the key bytes then
  start on a 16-byte boundary of the destination or 8 bytes past one), with
  one list that holds every value, with empty lists first and last; file
  streams one byte below, at and above the workgroup unit and over several
  units; partitions whose key bytes start at every offset mod 16 of the
  source; keys of a few hundred bytes; a source blob that neither starts nor
  ends on a 16-byte boundary.
* ``mr_mrl1_decode``: over the encoder's files: the row -> file and value ->
  file searches at the 255 / 256 / 257 block boundaries, zero-row files
  between the others, files with rows and no value, the value -> row index
  against ``np.repeat``, the ``rep`` words (the keys are read back through
  them), nothing written outside the output rows and values.

The kernels only move bits: the values carry NaNs with payloads, signed zeros,
infinities and the int64 extremes.
"""
import numpy as np
import pytest
import torch

from lua_mapreduce_1_amd import ops
from lua_mapreduce_1_amd.ops import _hip
from lua_mapreduce_1_amd.ops import keys as K
from lua_mapreduce_1_amd.runtime import codec, device as dev, job

pytestmark = pytest.mark.gpu

FILL = 0xA5
SHAPES = ("none", "odd", "even", "one", "ends")


def _unit() -> int:
    return int(_hip.lib().mr_mrl1_encode_unit())


def _values(rng, n: int) -> np.ndarray:
    """n words of random bits with the special values of i64 and f64 in front."""
    a = rng.integers(0, 2**64, n, dtype=np.uint64)
    sp = np.array([0x8000000000000000, 0x7FFFFFFFFFFFFFFF, 0, 0xFFFFFFFFFFFFFFFF, 0x7FF80000DEADBEEF,
                   0xFFF0000000000001, 0x7FF0000000000000, 0xFFF0000000000000, 0x0000000000000001], np.uint64)
    m = min(n, sp.size)
    a[:m] = sp[:m]
    return a


def _list_lens(rng, n: int, shape: str) -> list[int]:
    """Value counts of a file's n lists."""
    if shape == "none":
        return [0] * n
    if shape == "one":
        ln = [0] * n
        ln[n // 2] = int(rng.integers(1, 60))
        return ln
    ln = rng.integers(0, 5, n).tolist()
    if shape == "ends":
        ln[0] = ln[-1] = 0
        return ln
    if sum(ln) % 2 != (1 if shape == "odd" else 0):
        ln[n // 2] += 1
    if sum(ln) == 0:
        ln[n // 2] += 2
    return ln


def _table(rng, rows: list[int], key_lens: list[int], list_lens: list[int]):
    """Sorted columns of sum(rows) keys (partition p = the next rows[p] rows)
    with their lists, as order_lists leaves them, on the host."""
    n = sum(rows)
    assert len(key_lens) == len(list_lens) == n
    hi = rng.integers(0, 2**64, n, dtype=np.uint64)
    lo = rng.integers(0, 2**64, n, dtype=np.uint64)
    off = np.zeros(n + 1, np.int64)
    np.cumsum(key_lens, out=off[1:])
    loff = np.zeros(n + 1, np.int64)
    np.cumsum(list_lens, out=loff[1:])
    blob = rng.integers(0, 256, int(off[-1]), dtype=np.uint8)
    return hi, lo, off, blob, loff, _values(rng, int(loff[-1]))


def _want_files(tab, rows, code):
    hi, lo, off, blob, loff, lval = tab
    files, a = [], 0
    for n in rows:
        if n:
            b = a + n
            files.append(codec.encode_lists(hi[a:b], lo[a:b], off[a:b + 1] - off[a], blob[off[a]:off[b]],
                                            loff[a:b + 1] - loff[a], lval[loff[a]:loff[b]], code))
        a += n
    return files


def _t(a, gpu):
    return torch.from_numpy(np.ascontiguousarray(a)).to(gpu)


def _encode(gpu, tab, rows, pad: int, code: int = 0):
    """One launch over the non-empty partitions; the key blob lies ``pad``
    bytes past a 16-byte boundary inside a larger tensor.  The whole
    destination is compared with the host encoder's files."""
    hi, lo, off, blob, loff, lval = tab
    files = _want_files(tab, rows, code)
    starts = np.cumsum([0] + list(rows))[:-1]
    live = [p for p, n in enumerate(rows) if n]
    # places as the arena gives them: back to back at 4 mod 16 (4 .. 19 bytes between files)
    places, end = [], 16
    for f in files:
        o = (end + 15) // 16 * 16 + 4
        places.append(o)
        end = o + len(f)
    total = end + 64
    want = np.full(total, FILL, np.uint8)
    for o, f in zip(places, files):
        want[o:o + len(f)] = np.frombuffer(f, np.uint8)
    dst = torch.full((total,), FILL, dtype=torch.uint8, device=gpu)
    assert dst.data_ptr() % 16 == 0
    big = torch.full((blob.size + 48,), 0x5A, dtype=torch.uint8, device=gpu)
    assert big.data_ptr() % 16 == 0
    dblob = big[pad:pad + blob.size]
    dblob.copy_(torch.from_numpy(blob))
    dhi, dlo, doff, dloff = _t(hi.view(np.int64), gpu), _t(lo.view(np.int64), gpu), _t(off, gpu), _t(loff, gpu)
    dval = _t(np.concatenate([lval, np.zeros(1, np.uint64)]).view(np.int64), gpu)[:lval.size]
    unit = _unit()
    units = np.array([(len(f) + 4 + unit - 1) // unit for f in files], np.int64)
    ustart = np.zeros(len(files), np.int64)
    np.cumsum(units[:-1], out=ustart[1:])
    plan = np.concatenate([np.array([dst.data_ptr() + o for o in places], np.uint64).view(np.int64),
                           starts[live].astype(np.int64), np.array([rows[p] for p in live], np.int64), ustart])
    dplan = torch.from_numpy(plan).to(gpu)
    _hip.call("mr_mrl1_encode", _hip.ptr(dhi), _hip.ptr(dlo), _hip.ptr(doff), _hip.ptr(dloff), _hip.ptr(dval),
              int(dval.numel()), _hip.ptr(dblob), int(dblob.numel()), _hip.ptr(dplan), len(files), int(units.sum()),
              code, _hip.stream(gpu))
    got = dst.cpu().numpy()
    bad = np.flatnonzero(got != want)
    assert bad.size == 0, (f"{bad.size} wrong bytes, first at destination offset {int(bad[0])}; files at {places[:8]} "
                           f"of {[len(f) for f in files][:8]} bytes")
    assert bool((big[:pad] == 0x5A).all()) and bool((big[pad + blob.size:] == 0x5A).all())
    return files


def _key_lens(rng, n: int) -> list[int]:
    """Mostly short keys, some past 15 bytes, a few of some hundred bytes."""
    ln = rng.integers(1, 31, n)
    ln[rng.random(n) < 0.03] = int(rng.integers(200, 400))
    return ln.tolist()


def _layout_rows(layout: str) -> list[int]:
    if layout == "six":
        return [1, 2, 255, 256, 257, 3]
    if layout == "one":
        return [257]
    rows = [0] * 256
    rows[0], rows[17], rows[100], rows[101], rows[255] = 5, 1, 33, 4, 2
    return rows


def _shaped_table(rng, rows: list[int], first_shape: int):
    """A table whose p-th non-empty partition has the list shape
    SHAPES[(first_shape + p) % 5]; -> (table, the shapes used)."""
    lls, used, q = [], [], first_shape
    for n in rows:
        if n:
            s = SHAPES[q % len(SHAPES)]
            lls += _list_lens(rng, n, s)
            used.append(s)
            q += 1
    tab = _table(rng, rows, _key_lens(rng, sum(rows)), lls)
    return tab, used


# -- mr_mrl1_plan ---------------------------------------------------------------------------------
def _plan(gpu, counts, off, loff, n: int):
    nparts = len(counts)
    out = torch.full((3 * nparts + 3 + 8,), -7, dtype=torch.int64, device=gpu)
    dc, doff, dloff = _t(np.asarray(counts, np.int64), gpu), _t(off, gpu), _t(loff, gpu)
    _hip.call("mr_mrl1_plan", _hip.ptr(dc), _hip.ptr(doff), _hip.ptr(dloff), n, nparts, _hip.ptr(out), _hip.stream(gpu))
    got = out.cpu().numpy()
    assert (got[3 * nparts + 3:] == -7).all()  # the plan is 3 * nparts + 3 words, no more
    return got[:3 * nparts + 3]


@pytest.mark.parametrize("layout", ["six", "one", "sparse256"])
def test_mrl1_plan_matches_numpy(gpu, layout):
    rng = np.random.default_rng(len(layout))
    rows = _layout_rows(layout)
    (hi, lo, off, blob, loff, lval), _used = _shaped_table(rng, rows, 1)
    n, nparts = sum(rows), len(rows)
    got = _plan(gpu, rows, off, loff, n)
    b = np.concatenate([[0], np.cumsum(rows)])
    want = np.concatenate([rows, off[b[1:]] - off[b[:-1]], loff[b[1:]] - loff[b[:-1]], [off[n], loff[n], n]])
    assert np.array_equal(got, want)
    parts, starts, r, nb, nv, sizes = dev.mrl1_file_plan(got, n, nparts, blob.size, lval.size)
    assert parts.tolist() == [p for p, x in enumerate(rows) if x] and starts.tolist() == b[:-1][parts].tolist()
    assert sizes.tolist() == [len(f) for f in _want_files((hi, lo, off, blob, loff, lval), rows, 0)]
    assert dev.mrl1_file_plan(got, n, nparts, blob.size - 1, lval.size) is None
    if lval.size:
        assert dev.mrl1_file_plan(got, n, nparts, blob.size, lval.size - 1) is None
    # counts that sum past n: the bounds are clamped to n (nothing outside the n + 1 offsets is read:
    # the tensors end there), the sum tells, and the host refuses the plan
    for bump in (1, 1 << 40):
        over = list(rows)
        over[len(over) // 2] += bump
        g2 = _plan(gpu, over, off, loff, n)
        b2 = np.minimum(np.concatenate([[0], np.cumsum(over)]), n)
        w2 = np.concatenate([over, off[b2[1:]] - off[b2[:-1]], loff[b2[1:]] - loff[b2[:-1]], [off[n], loff[n], n + bump]])
        assert np.array_equal(g2, w2)
        assert dev.mrl1_file_plan(g2, n, nparts, blob.size, lval.size) is None
    short = list(rows)
    short[-1] -= 1
    g3 = _plan(gpu, short, off, loff, n)
    assert g3[-1] == n - 1 and dev.mrl1_file_plan(g3, n, nparts, blob.size, lval.size) is None


# -- mr_mrl1_encode -------------------------------------------------------------------------------
@pytest.mark.parametrize("pad", [0, 5])
@pytest.mark.parametrize("layout", ["six", "one", "sparse256"])
@pytest.mark.parametrize("first_shape", range(len(SHAPES)), ids=SHAPES)
def test_mrl1_encode_matches_host_encoder(gpu, first_shape, layout, pad):
    rng = np.random.default_rng(first_shape * 7 + len(layout) + pad)
    rows = _layout_rows(layout)
    tab, used = _shaped_table(rng, rows, first_shape)
    files = _encode(gpu, tab, rows, pad, code=first_shape % 2)
    assert len(files) == sum(1 for n in rows if n)
    nvs = [codec.decode_lists(f)["list_val"].size for f in files]
    for s, nv in zip(used, nvs):
        assert (nv == 0) if s == "none" else (nv % 2 == 1) if s == "odd" else (nv % 2 == 0) if s == "even" else True
    if layout != "one":
        assert set(used) == set(SHAPES)


def test_mrl1_encode_every_source_offset_of_the_key_bytes(gpu):
    """33 partitions of one or two rows whose key bytes add up to 1 mod 16:
    partition p's bytes start p mod 16 past the blob's own offset, with keys
    longer than a 16-byte vector; blob offsets 0, 3 and 14 (the first
    partition's vector would start before the blob, the last one's end
    behind it).  Odd and even value counts alternate, so both byte heads
    meet every source offset."""
    for pad in (0, 3, 14):
        for parity in (0, 1):
            rng = np.random.default_rng(pad + parity)
            rows = [1 + p % 2 for p in range(33)]
            lens, lls = [], []
            for p, n in enumerate(rows):
                lens += [17 + 16 * int(rng.integers(0, 12))] if n == 1 else [40, 9 + 16 * int(rng.integers(0, 3))]
                lls += [(p // 2 + parity) % 2 + 2 * int(rng.integers(0, 3))] + [2] * (n - 1)
            tab = _table(rng, rows, lens, lls)
            off = tab[2]
            starts = np.cumsum([0] + rows)[:-1]
            assert sorted({int(off[a] + pad) % 16 for a in starts}) == list(range(16))
            assert (off[-1] + pad) % 16 != 0
            files = _encode(gpu, tab, rows, pad)
            assert {codec.decode_lists(f)["list_val"].size % 2 for f in files} == {0, 1}


@pytest.mark.parametrize("nv_parity", [0, 1], ids=["even_nv", "odd_nv"])
def test_mrl1_encode_round_the_unit_size(gpu, nv_parity):
    """Files whose stream (the file and the 4 bytes before it) is one byte
    short of a workgroup unit, exactly one, one byte more, and a file of
    several units (unit boundaries inside the words, the values and the key
    bytes)."""
    unit = _unit()
    rng = np.random.default_rng(nv_parity)
    n = 101
    rows, lens, lls = [], [], []
    for target in (unit - 1, unit, unit + 1):
        ll = rng.integers(0, 4, n).tolist()
        if sum(ll) % 2 != nv_parity:
            ll[7] += 1
        nb = target - 4 - (52 + 32 * n + 8 * sum(ll))
        assert nb >= n
        ln = [nb // n] * n
        ln[0] += nb - sum(ln)
        assert max(ln) < 400
        rows.append(n)
        lens += ln
        lls += ll
    big = 1501
    rows.append(big)
    lens += _key_lens(rng, big)
    bl = rng.integers(0, 3, big).tolist()
    bl[3] += 2000 + nv_parity - sum(bl) % 2  # (a list over a unit boundary of its own)
    lls += bl
    tab = _table(rng, rows, lens, lls)
    files = _encode(gpu, tab, rows, 7, code=1)
    assert [len(f) + 4 for f in files[:3]] == [unit - 1, unit, unit + 1]
    assert len(files[3]) > 3 * unit
    assert all(codec.decode_lists(f)["list_val"].size % 2 == nv_parity for f in files[:3])


# -- mr_mrl1_decode -------------------------------------------------------------------------------
def _file_tables(rng, specs):
    """specs: per file (rows, shape | list of list lengths) -> one table whose
    partitions are the files (zero-row files: empty partitions)."""
    rows, lls = [], []
    for n, shape in specs:
        rows.append(n)
        lls += shape if isinstance(shape, list) else (_list_lens(rng, n, shape) if n else [])
    return rows, _table(rng, rows, _key_lens(rng, sum(rows)), lls)


def _decode_case(gpu, rng, specs, code: int = 0):
    """The device encoder's files (every file of the buffer, the zero-row
    ones as the 52-byte file the host encoder makes), decoded by one launch."""
    rows, tab = _file_tables(rng, specs)
    live = _encode(gpu, tab, rows, 5, code) if any(rows) else []  # (the device's bytes are these)
    z64, zi = np.zeros(0, np.uint64), np.zeros(1, np.int64)
    empty = codec.encode_lists(z64, z64, zi, np.zeros(0, np.uint8), zi, np.zeros(0, np.int64), code)
    it = iter(live)
    files = [next(it) if n else empty for n in rows]
    lens = [len(b) for b in files]
    bases, total = job._aligned_bases(lens)
    host = np.full(max(total, 16), 0xEE, np.uint8)
    for o, b in zip(bases, files):
        host[o:o + len(b)] = np.frombuffer(b, np.uint8)
    buf = torch.from_numpy(host).to(gpu)
    cols = [codec.decode_lists(b) for b in files]
    rep, vrow, r0, keys = [], [], 0, []
    for c, b, base in zip(cols, files, bases):
        kb = base + len(b) - int(c["key_blob"].size)  # the key bytes end the file
        ko = c["key_off"]
        n = int(c["hi"].size)
        rep += [K.make_rep(kb + int(ko[i]), int(ko[i + 1] - ko[i])) for i in range(n)]
        blob = c["key_blob"].tobytes()
        keys += [blob[int(ko[i]):int(ko[i + 1])] for i in range(n)]
        vrow.append(np.repeat(np.arange(n, dtype=np.int64), np.diff(c["list_off"])) + r0)
        r0 += n
    want = (np.concatenate([c["hi"] for c in cols]), np.concatenate([c["lo"] for c in cols]), np.array(rep, np.uint64),
            np.concatenate([c["list_val"].view(np.uint64) for c in cols]), np.concatenate(vrow))
    nbs = [int(c["key_blob"].size) for c in cols]
    nvs = [int(c["list_val"].size) for c in cols]
    return buf, bases, rows, lens, nbs, nvs, want, keys


DECODE_CASES = {
    "one_row": [(1, [3])],
    "one_row_no_value": [(1, [0])],
    "blocks": [(255, "odd"), (256, "even"), (257, "ends")],
    "value_blocks": [(3, [255, 0, 0]), (2, [0, 256]), (4, [0, 257, 0, 1]), (1, [255])],
    "zero_row_files": [(0, "none"), (7, "ends"), (0, "none"), (300, "one"), (0, "none")],
    "rows_without_values": [(5, "odd"), (260, "none"), (3, "none"), (9, "even"), (4, "none")],
    "no_values_at_all": [(255, "none"), (2, "none")],
    "more_values_than_rows": [(2, [700, 1]), (1, [0]), (3, [0, 0, 513])],
    "nothing": [(0, "none")],
}


@pytest.mark.parametrize("case", list(DECODE_CASES))
def test_mrl1_decode_matches_host_decoder(gpu, case):
    rng = np.random.default_rng(len(case))
    buf, bases, rows, lens, nbs, nvs, want, keys = _decode_case(gpu, rng, DECODE_CASES[case], code=len(case) % 2)
    hi, lo, rep, vbits, vrow = job._decode_list_files(buf, bases, rows, lens, nbs, nvs)
    n, nv = sum(rows), sum(nvs)
    assert hi.numel() == lo.numel() == rep.numel() == n and vbits.numel() == vrow.numel() == nv
    for g, w in zip((hi, lo, rep, vbits), want[:4]):
        assert np.array_equal(g.cpu().numpy().view(np.uint64), w)
    assert np.array_equal(vrow.cpu().numpy(), want[4])
    if n == 0:
        return
    # the keys read back through rep: random hi / lo bits say nothing about a key, so every row is
    # marked long and its bytes come from buf alone
    off, blob = ops.gather_key_bytes(hi, lo | 0xFF, rep, buf)
    off, blob = off.cpu().numpy(), blob.cpu().numpy().tobytes()
    assert [blob[int(off[i]):int(off[i + 1])] for i in range(n)] == keys


@pytest.mark.parametrize("case", ["blocks", "value_blocks", "rows_without_values", "no_values_at_all",
                                  "more_values_than_rows"])
def test_mrl1_decode_writes_only_its_rows_and_values(gpu, case):
    """The kernel called directly, each output inside a larger tensor of a
    sentinel: 64 elements before and after the rows / values stay as they
    were."""
    rng = np.random.default_rng(3)
    buf, bases, rows, lens, nbs, nvs, want, _keys = _decode_case(gpu, rng, DECODE_CASES[case])
    job._check_mrl1_layout(buf.numel(), bases, rows, lens, nbs, nvs)
    n, nv, pad = sum(rows), sum(nvs), 64
    rstart = np.zeros(len(rows) + 1, np.int64)
    np.cumsum(rows, out=rstart[1:])
    vstart = np.zeros(len(rows) + 1, np.int64)
    np.cumsum(nvs, out=vstart[1:])
    meta = torch.from_numpy(np.concatenate([np.asarray(bases, np.int64), rstart, vstart])).to(gpu)
    sent = -0x0123456789ABCDEF
    outs = [torch.full((m + 2 * pad,), sent, dtype=torch.int64, device=gpu) for m in (n, n, n, nv, nv)]
    _hip.call("mr_mrl1_decode", _hip.ptr(buf), _hip.ptr(meta), len(rows), n, nv,
              *[_hip.ptr(o[pad:pad + m]) for o, m in zip(outs, (n, n, n, nv, nv))], _hip.stream(gpu))
    for o, w, m in zip(outs, want, (n, n, n, nv, nv)):
        h = o.cpu().numpy()
        assert (h[:pad] == sent).all() and (h[pad + m:] == sent).all()
        assert np.array_equal(h[pad:pad + m].view(np.uint64), np.asarray(w).view(np.uint64))
    # no rows, no files: nothing is launched, nothing written
    fresh = [torch.full((8,), sent, dtype=torch.int64, device=gpu) for _ in range(5)]
    for nfiles, nrows, nvals in ((len(rows), 0, 0), (0, 0, 0), (0, 5, 5)):
        _hip.call("mr_mrl1_decode", _hip.ptr(buf), _hip.ptr(meta), nfiles, nrows, nvals, *[_hip.ptr(x) for x in fresh],
                  _hip.stream(gpu))
    assert all(bool((x == sent).all()) for x in fresh)
