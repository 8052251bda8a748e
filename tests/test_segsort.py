"""ops/segments.quantiles on CPU tensors (the specification of the GPU pick
kernel) against a per-list loop, and median unchanged on top of it."""
import numpy as np
import pytest
import torch

from lua_mapreduce_1_amd.ops import segments as S


@pytest.mark.parametrize("dtype", [np.int64, np.float64])
def test_quantiles_cpu_match_loop(dtype):
    qs = (0.0, 0.5, 0.9, 0.99, 1.0)
    off = np.array([0, 0, 1, 3, 10, 10, 75], dtype=np.int64)
    v = (np.random.default_rng(5).normal(size=75) * 100).astype(dtype)
    got = S.quantiles(torch.from_numpy(off), torch.from_numpy(v), qs).numpy()
    exp = np.full((6, len(qs)), np.nan)
    for s in range(6):
        sv = np.sort(v[off[s]:off[s + 1]]).astype(np.float64)
        for j, q in enumerate(qs):
            if sv.size:
                pos = np.float64(sv.size - 1) * q
                lo, hi = int(np.floor(pos)), int(np.ceil(pos))
                exp[s, j] = sv[lo] + (sv[hi] - sv[lo]) * (pos - lo)
    assert np.array_equal(got.view(np.uint64), exp.view(np.uint64))
    pre = S.sort(torch.from_numpy(off), torch.from_numpy(v))
    assert np.array_equal(S.quantiles(torch.from_numpy(off), pre, qs, sorted=True).numpy(), got, equal_nan=True)


def test_median_even_odd_empty():
    off = torch.tensor([0, 4, 7, 7])
    val = torch.tensor([4, 1, 3, 2, 9, 7, 8])
    got = S.median(off, val)
    assert got.dtype == torch.float64 and got[:2].tolist() == [2.5, 8.0] and bool(torch.isnan(got[2]))


def test_sort_tile_is_exported():
    assert S.SORT_TILE is None or (S.SORT_TILE >= 64 and S.SORT_TILE & (S.SORT_TILE - 1) == 0)
