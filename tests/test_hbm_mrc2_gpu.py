"""The MRC2 device codec of ``hbm`` storage (csrc/hip/ipc.hip) against the
host codec (``codec.encode_columns`` / ``codec.decode_columns``).

* ``mr_mrc2_encode``: every non-empty partition's file of a sorted column set
  in ONE launch, into a destination filled with a sentinel: the whole
  destination is compared, so every byte outside the files must keep the
  fill.  Column sets with 8- and 4-byte values (an f32 column of odd n puts
  the later columns and the key bytes at 4 mod 8), files of 1, 2, 255, 256
  and 257 rows, 1, 6 and 256 partitions, file streams one byte below, at and
  above the workgroup unit and over several units, partitions whose key
  bytes start at every offset mod 16 of the source, keys of up to a few
  hundred bytes, a source blob that neither starts nor ends on a 16-byte
  boundary.
* ``mr_mrc2_decode``: the row -> file search at the 255 / 256 / 257 block
  boundaries, zero-row files, columns at 4 mod 8, the ``rep`` words (the keys
  are read back through them), nothing written outside the output rows.

The kernels only move bits: the values carry NaNs with payloads, signed zeros,
infinities and the int64 extremes.
"""
import ctypes

import numpy as np
import pytest
import torch

from lua_mapreduce_1_amd import ops
from lua_mapreduce_1_amd.ops import _hip
from lua_mapreduce_1_amd.ops import keys as K
from lua_mapreduce_1_amd.runtime import codec, job

pytestmark = pytest.mark.gpu

FILL = 0xA5
I64, F64, F32 = np.int64, np.float64, np.float32
COLSETS = {"f64": (F64,), "i64": (I64,), "f32": (F32,), "f32_f64_i64": (F32, F64, I64), "f32_f32_i64": (F32, F32, I64),
           "eight": (F32, I64, F64, F32, F32, F64, I64, F32)}
_WIDTH = {I64: 8, F64: 8, F32: 4}


def _unit() -> int:
    return int(_hip.lib().mr_mrc2_encode_unit())


def _column(rng, dt, n: int) -> np.ndarray:
    """n values of random bits (NaNs of any payload among the floats) with the
    special values of the dtype in front."""
    if dt is F32:
        a = rng.integers(0, 2**32, n, dtype=np.uint32)
        sp = np.array([0x7FC0BEEF, 0xFFC00001, 0x80000000, 0x00000000, 0x7F800000, 0xFF800000, 0x00000001], np.uint32)
    else:
        a = rng.integers(0, 2**64, n, dtype=np.uint64)
        if dt is I64:
            sp = np.array([0x8000000000000000, 0x7FFFFFFFFFFFFFFF, 0, 0xFFFFFFFFFFFFFFFF], np.uint64)
        else:
            sp = np.array([0x7FF80000DEADBEEF, 0xFFF0000000000001, 0x8000000000000000, 0, 0x7FF0000000000000,
                           0xFFF0000000000000, 0x0000000000000001], np.uint64)
    m = min(n, sp.size)
    a[:m] = sp[:m]
    return a.view(dt)


def _table(rng, dts, rows: list[int], key_lens: list[int]):
    """Sorted columns of sum(rows) keys (partition p = the next rows[p] rows)
    as order_fold leaves them, on the host."""
    n = sum(rows)
    assert len(key_lens) == n
    hi = rng.integers(0, 2**64, n, dtype=np.uint64)
    lo = rng.integers(0, 2**64, n, dtype=np.uint64)
    cols = [_column(rng, dt, n) for dt in dts]
    off = np.zeros(n + 1, np.int64)
    np.cumsum(key_lens, out=off[1:])
    blob = rng.integers(0, 256, int(off[-1]), dtype=np.uint8)
    return hi, lo, cols, off, blob


def _want_files(tab, rows):
    hi, lo, cols, off, blob = tab
    files, a = [], 0
    for n in rows:
        if n:
            b = a + n
            files.append(codec.encode_columns(hi[a:b], lo[a:b], [c[a:b] for c in cols], off[a:b + 1] - off[a],
                                              blob[off[a]:off[b]]))
        a += n
    return files


def _encode(gpu, tab, rows, pad: int):
    """One launch over the non-empty partitions; the key blob lies ``pad``
    bytes past a 16-byte boundary inside a larger tensor.  The whole
    destination is compared with the host encoder's files."""
    hi, lo, cols, off, blob = tab
    files = _want_files(tab, rows)
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
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(gpu)  # noqa: E731
    dhi, dlo, doff = t(hi.view(np.int64)), t(lo.view(np.int64)), t(off)
    dcols = [t(c) for c in cols]
    unit = _unit()
    units = np.array([(len(f) + 4 + unit - 1) // unit for f in files], np.int64)
    ustart = np.zeros(len(files), np.int64)
    np.cumsum(units[:-1], out=ustart[1:])
    plan = np.concatenate([np.array([dst.data_ptr() + o for o in places], np.uint64).view(np.int64),
                           starts[live].astype(np.int64), np.array([rows[p] for p in live], np.int64), ustart])
    dplan = torch.from_numpy(plan).to(gpu)
    _hip.call("mr_mrc2_encode", _hip.ptr(dhi), _hip.ptr(dlo), _hip.ptr(doff), _hip.ptr(dblob), int(dblob.numel()),
              ctypes.byref(_hip.mrc2_cols(dcols)), _hip.ptr(dplan), len(files), int(units.sum()), _hip.stream(gpu))
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


@pytest.mark.parametrize("pad", [0, 5])
@pytest.mark.parametrize("layout", ["six", "one", "sparse256"])
@pytest.mark.parametrize("colset", list(COLSETS))
def test_mrc2_encode_matches_host_encoder(gpu, colset, layout, pad):
    rng = np.random.default_rng(len(colset) * 7 + len(layout) + pad)
    if layout == "six":
        rows = [1, 2, 255, 256, 257, 3]
    elif layout == "one":
        rows = [257]
    else:
        rows = [0] * 256
        rows[0], rows[17], rows[100], rows[255] = 5, 1, 33, 2
    tab = _table(rng, COLSETS[colset], rows, _key_lens(rng, sum(rows)))
    files = _encode(gpu, tab, rows, pad)
    assert len(files) == sum(1 for n in rows if n)


@pytest.mark.parametrize("colset", ["f64", "f32", "f32_f64_i64", "eight"])
def test_mrc2_encode_every_source_offset_of_the_key_bytes(gpu, colset):
    """33 partitions of one or two rows whose key bytes add up to 1 mod 16:
    partition p's bytes start p mod 16 past the blob's own offset, with keys
    longer than a 16-byte vector; blob offsets 0, 3 and 14 (the first
    partition's vector would start before the blob, the last one's end
    behind it)."""
    for pad in (0, 3, 14):
        rng = np.random.default_rng(pad)
        rows = [1 + p % 2 for p in range(33)]
        lens = []
        for n in rows:
            lens += [17 + 16 * int(rng.integers(0, 12))] if n == 1 else [40, 9 + 16 * int(rng.integers(0, 3))]
        tab = _table(rng, COLSETS[colset], rows, lens)
        off = tab[3]
        starts = np.cumsum([0] + rows)[:-1]
        assert sorted({int(off[a] + pad) % 16 for a in starts}) == list(range(16))
        assert (off[-1] + pad) % 16 != 0
        _encode(gpu, tab, rows, pad)


@pytest.mark.parametrize("colset", list(COLSETS))
def test_mrc2_encode_round_the_unit_size(gpu, colset):
    """Files whose stream (the file and the 4 bytes before it) is one byte
    short of a workgroup unit, exactly one, one byte more, and a file of
    several units with an odd row count (unit boundaries inside the words,
    the value region at 4 mod 8 and the key bytes)."""
    unit = _unit()
    dts = COLSETS[colset]
    w = sum(_WIDTH[dt] for dt in dts)
    rng = np.random.default_rng(w)
    n = 101
    rows, lens = [], []
    for target in (unit - 1, unit, unit + 1):
        nb = target - 4 - (44 + 24 * n + n * w)
        assert nb >= n
        ln = [nb // n] * n
        ln[0] += nb - sum(ln)
        assert max(ln) < 400
        rows.append(n)
        lens += ln
    big = 2001
    rows.append(big)
    lens += _key_lens(rng, big)
    tab = _table(rng, dts, rows, lens)
    files = _encode(gpu, tab, rows, 7)
    assert [len(f) + 4 for f in files[:3]] == [unit - 1, unit, unit + 1]
    assert len(files[3]) > 3 * unit


# -- mr_mrc2_decode -----------------------------------------------------------------
def _random_file(rng, dts, n: int):
    lens = _key_lens(rng, n)
    hi, lo, cols, off, blob = _table(rng, dts, [n], lens)
    keys = [blob[off[i]:off[i + 1]].tobytes() for i in range(n)]
    return codec.encode_columns(hi, lo, cols, off, blob), keys


def _layout(files, gpu):
    lens = [len(b) for b in files]
    bases, total = job._aligned_bases(lens)
    host = np.full(max(total, 16), 0xEE, np.uint8)
    for o, b in zip(bases, files):
        host[o:o + len(b)] = np.frombuffer(b, np.uint8)
    return torch.from_numpy(host).to(gpu), bases, lens


def _expected(files, bases):
    cols = [codec.decode_columns(b) for b in files]
    rep = []
    for c, b, base in zip(cols, files, bases):
        kb = base + len(b) - int(c["key_blob"].size)  # the key bytes end the file
        ko = c["key_off"]
        rep += [K.make_rep(kb + int(ko[i]), int(ko[i + 1] - ko[i])) for i in range(int(c["hi"].size))]
    k = len(cols[0]["cols"])
    return (np.concatenate([c["hi"] for c in cols]), np.concatenate([c["lo"] for c in cols]), np.array(rep, np.uint64),
            [np.concatenate([c["cols"][j] for c in cols]) for j in range(k)])


def _codes(dts) -> list[int]:
    return [codec._DT_CODE[np.dtype(dt)] for dt in dts]


def _bits(a: np.ndarray) -> np.ndarray:
    return a.view(np.uint32 if a.dtype.itemsize == 4 else np.uint64)


@pytest.mark.parametrize("rows", [[1], [255, 256, 257], [0, 7, 0, 300, 0], [0]], ids=lambda v: "-".join(map(str, v)))
@pytest.mark.parametrize("colset", list(COLSETS))
def test_mrc2_decode_matches_host_decoder(gpu, colset, rows):
    dts = COLSETS[colset]
    rng = np.random.default_rng(sum(rows) + len(dts))
    made = [_random_file(rng, dts, n) for n in rows]
    files = [m[0] for m in made]
    keys = [k for m in made for k in m[1]]
    buf, bases, lens = _layout(files, gpu)
    heads = [codec.decode_columns(b) for b in files]
    nbs = [int(h["key_blob"].size) for h in heads]
    hi, lo, rep, vals = job._decode_cols_files(buf, bases, rows, lens, nbs, [_codes(dts)] * len(rows), _codes(dts))
    w_hi, w_lo, w_rep, w_vals = _expected(files, bases)
    n = sum(rows)
    assert hi.numel() == lo.numel() == rep.numel() == n and all(v.numel() == n for v in vals)
    assert np.array_equal(hi.cpu().numpy().view(np.uint64), w_hi)
    assert np.array_equal(lo.cpu().numpy().view(np.uint64), w_lo)
    assert np.array_equal(rep.cpu().numpy().view(np.uint64), w_rep)
    for v, w, dt in zip(vals, w_vals, dts):
        g = v.cpu().numpy()
        assert g.dtype == np.dtype(dt) and np.array_equal(_bits(g), _bits(w))
    if n == 0:
        return
    # the keys read back through rep: random hi / lo bits say nothing about a key, so every row is
    # marked long and its bytes come from buf alone
    off, blob = ops.gather_key_bytes(hi, lo | 0xFF, rep, buf)
    off, blob = off.cpu().numpy(), blob.cpu().numpy().tobytes()
    assert [blob[int(off[i]):int(off[i + 1])] for i in range(n)] == keys


@pytest.mark.parametrize("colset", ["f32", "f32_f64_i64", "eight"])
def test_mrc2_decode_writes_only_its_rows(gpu, colset):
    """The kernel called directly, each output column inside a larger tensor
    of a sentinel: 64 elements before and after the n rows stay as they were
    (n = 513: a last block of one row; a zero-row file in the middle)."""
    dts = COLSETS[colset]
    rng = np.random.default_rng(3)
    rows = [255, 0, 258]
    files = [_random_file(rng, dts, n)[0] for n in rows]
    buf, bases, lens = _layout(files, gpu)
    nbs = [int(codec.decode_columns(b)["key_blob"].size) for b in files]
    job._check_mrc2_layout(buf.numel(), bases, rows, lens, nbs, [_codes(dts)] * 3, _codes(dts))
    n, pad = sum(rows), 64
    rstart = np.zeros(len(rows) + 1, np.int64)
    np.cumsum(rows, out=rstart[1:])
    meta = torch.from_numpy(np.concatenate([np.asarray(bases, np.int64), rstart])).to(gpu)
    sent64, sent32 = -0x0123456789ABCDEF, 0x5EA15EA1
    keys = [torch.full((n + 2 * pad,), sent64, dtype=torch.int64, device=gpu) for _ in range(3)]
    outs = []
    for dt in dts:
        if dt is F32:
            outs.append(torch.full((n + 2 * pad,), sent32, dtype=torch.int32, device=gpu).view(torch.float32))
        else:
            o = torch.full((n + 2 * pad,), sent64, dtype=torch.int64, device=gpu)
            outs.append(o.view(torch.float64) if dt is F64 else o)
    views = [o[pad:pad + n] for o in outs]
    cs = _hip.mrc2_cols(views)
    _hip.call("mr_mrc2_decode", _hip.ptr(buf), _hip.ptr(meta), len(rows), n, *[_hip.ptr(x[pad:pad + n]) for x in keys],
              ctypes.byref(cs), _hip.stream(gpu))
    w_hi, w_lo, w_rep, w_vals = _expected(files, bases)

    def check(o, w):
        h = _bits(o.cpu().numpy())
        sent = np.uint32(sent32) if h.dtype == np.uint32 else np.int64(sent64).astype(np.uint64)
        assert (h[:pad] == sent).all() and (h[pad + n:] == sent).all()
        assert np.array_equal(h[pad:pad + n], _bits(w))

    for o, w in zip(keys + outs, [w_hi, w_lo, w_rep] + w_vals):
        check(o, w)
    # no rows, no files: nothing is launched, nothing written
    fresh = [torch.full((8,), sent64, dtype=torch.int64, device=gpu) for _ in range(4)]
    one = _hip.mrc2_cols([fresh[3]])
    for nfiles, nrows in ((len(rows), 0), (0, 0), (0, 5)):
        _hip.call("mr_mrc2_decode", _hip.ptr(buf), _hip.ptr(meta), nfiles, nrows, *[_hip.ptr(x) for x in fresh[:3]],
                  ctypes.byref(one), _hip.stream(gpu))
    assert all(bool((x == sent64).all()) for x in fresh)
