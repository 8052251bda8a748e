"""The segmented merge sort and the multi-quantile pick on the GPU
(csrc/hip/segsort.hip through ops/segments.sort / quantiles) against plain
NumPy per list, compared as raw 64-bit patterns: equal order keys have equal
bits, so the expected output is unique.  The layouts are the smallest at which
each mechanism can fail (T = the kernel's tile)."""
import numpy as np
import pytest
import torch

from lua_mapreduce_1_amd.ops import segments as S

pytestmark = pytest.mark.gpu

SIGN = np.uint64(1 << 63)
LAYOUTS = {
    "short": lambda T: [0, 0, 1, 2, 3, 0, 63, 64, 65, 1, 0],
    "tile": lambda T: [T],
    "tile_split": lambda T: [T - 1, 1],
    "spill": lambda T: [T + 1],
    "one_then_tile": lambda T: [1, T],
    "three_pieces": lambda T: [5, 2 * T + 3, 7],
    "parities": lambda T: [T // 2, 5 * T + 1, 3, 0, T - 4],
    "whole_tiles": lambda T: [3 * T],
    "staggered": lambda T: [T // 2 + 1] * 6,
}
F64_EDGES = np.array([0x0000000000000000, 0x8000000000000000, 0x7FF0000000000000, 0xFFF0000000000000,
                      0x0000000000000001, 0x800FFFFFFFFFFFFF, 0x7FF8000000000000, 0xFFF8000000000000,
                      0x7FF8000000000123, 0xFFF0000000000123, 0x3FF0000000000000, 0xBFF0000000000000], dtype=np.uint64)
I64_EDGES = np.array([-(1 << 63), (1 << 63) - 1, -1, 0, 1], dtype=np.int64)


def order_key(v: np.ndarray) -> np.ndarray:
    b = v.view(np.uint64)
    if v.dtype == np.float64:
        return np.where(b & SIGN != 0, ~b, b ^ SIGN)
    return b ^ SIGN


def values(kind: str, n: int, seed: int) -> np.ndarray:
    rng = np.random.default_rng(seed)
    if kind == "i64":
        return np.where(rng.random(n) < 0.3, rng.choice(I64_EDGES, n), rng.integers(-(1 << 63), (1 << 63) - 1, n))
    if kind == "f64":
        return np.where(rng.random(n) < 0.3, rng.choice(F64_EDGES, n).view(np.float64), rng.normal(size=n))
    if kind == "ties":
        return rng.integers(0, 8, n)
    return np.arange(n, dtype=np.int64) if kind == "asc" else np.arange(n, 0, -1, dtype=np.int64)


def expected(off, v, descending=False):
    out = v.copy()
    for b, e in zip(off[:-1], off[1:]):
        k = order_key(v[b:e])
        out[b:e] = v[b:e][np.argsort(~k if descending else k, kind="stable")]
    return out


def csr(lens):
    return np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)


def run_sort(gpu, off, v, descending=False):
    got = S.sort(torch.from_numpy(off).to(gpu), torch.from_numpy(v).to(gpu), descending=descending)
    assert got.dtype == torch.from_numpy(v).dtype
    return got.cpu().numpy()


@pytest.mark.parametrize("kind", ["i64", "f64", "ties", "asc", "desc"])
@pytest.mark.parametrize("layout", sorted(LAYOUTS))
def test_sort_matches_numpy(gpu, layout, kind):
    off = csr(LAYOUTS[layout](S.SORT_TILE))
    v = values(kind, int(off[-1]), seed=len(layout))
    got = run_sort(gpu, off, v)
    assert np.array_equal(got.view(np.uint64), expected(off, v).view(np.uint64))


@pytest.mark.parametrize("kind", ["i64", "f64"])
@pytest.mark.parametrize("layout", ["short", "parities"])
def test_sort_descending(gpu, layout, kind):
    off = csr(LAYOUTS[layout](S.SORT_TILE))
    v = values(kind, int(off[-1]), seed=7)
    got = run_sort(gpu, off, v, descending=True)
    assert np.array_equal(got.view(np.uint64), expected(off, v, True).view(np.uint64))


def test_empty_inputs(gpu):
    none = torch.zeros(0, dtype=torch.float64, device=gpu)
    for off in (torch.zeros(1, dtype=torch.int64, device=gpu), torch.zeros(4, dtype=torch.int64, device=gpu)):
        assert S.sort(off, none).numel() == 0
        q = S.quantiles(off, none, (0.5, 0.9))
        assert q.shape == (off.numel() - 1, 2) and bool(torch.isnan(q).all())


def quantiles_loop(off, v, qs):
    """The specification, one list and one q at a time (every operation rounded on its own)."""
    out = np.full((len(off) - 1, len(qs)), np.nan)
    for s, (b, e) in enumerate(zip(off[:-1], off[1:])):
        if e > b:
            sv = np.sort(v[b:e]).astype(np.float64)
            for j, q in enumerate(qs):
                pos = np.float64(e - b - 1) * np.float64(q)
                lo, hi = int(np.floor(pos)), int(np.ceil(pos))
                out[s, j] = sv[lo] + (sv[hi] - sv[lo]) * (pos - np.float64(lo))
    return out


@pytest.mark.parametrize("kind", ["i64", "f64"])
@pytest.mark.parametrize("layout", ["short", "three_pieces", "parities"])
def test_quantiles_bit_equal(gpu, layout, kind):
    qs = (0.0, 0.5, 0.9, 0.99, 1.0)
    off = csr(LAYOUTS[layout](S.SORT_TILE))
    rng = np.random.default_rng(3)
    n = int(off[-1])
    v = rng.normal(size=n) * 1e3 if kind == "f64" else rng.integers(-10**12, 10**12, n)
    o, t = torch.from_numpy(off).to(gpu), torch.from_numpy(v).to(gpu)
    got = S.quantiles(o, t, qs)
    assert got.dtype == torch.float64 and got.shape == (len(off) - 1, len(qs))
    assert np.array_equal(got.cpu().numpy().view(np.uint64), quantiles_loop(off, v, qs).view(np.uint64))
    assert torch.equal(S.quantiles(o, S.sort(o, t), qs, sorted=True).view(torch.int64), got.view(torch.int64))
    assert torch.equal(S.quantile(o, t, 0.9).view(torch.int64), got[:, 2].contiguous().view(torch.int64))
