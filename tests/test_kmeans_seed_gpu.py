"""The k-means|| seeding kernels (csrc/hip/kmeans_seed.hip) against the float64
numpy reference and bounds of test_kmeans_seed.py, at the smallest shapes at
which each part can go wrong; the sampling against the CPU specification, bit
for bit; and examples/KMeans with init_method="kmeans||" on cuda:0."""
import numpy as np
import pytest
import torch

from test_kmeans import blobs
from test_kmeans_seed import run_min_dist, seed_job_checks, seed_reference

pytestmark = pytest.mark.gpu

SHAPES = [(1, 1, 1, "fp32"), (17, 5, 17, "fp32"), (65, 64, 33, "fp32"),  # tails, one and two MFMA tiles
          (1000, 130, 15, "fp32"),    # d no multiple of 4, two d-chunks
          (257, 512, 3, "fp32"),      # d at the limit
          (300, 4, 5000, "fp32"),     # more candidates than MAX_K, many tiles
          (100_000, 8, 5, "fp32"),    # several super-tiles per workgroup
          (1000, 72, 130, "bf16")]    # widened points, the one-tile-per-wave variant, three candidate tiles
GPU_JOB_SEED = 5  # naive's smallest selection margin at this seed: asserted in seed_job_checks


@pytest.mark.parametrize("n,d,m,dtype", SHAPES)
def test_min_dist_shapes(gpu, n, d, m, dtype):
    X, C = blobs(n, d, m)
    x = torch.from_numpy(X)
    if dtype == "bf16":
        x = x.to(torch.bfloat16)
        X = x.float().numpy()  # the reference sees the rounded points
    ref = seed_reference(X, C)
    phi = run_min_dist(gpu, x, C, ref)
    assert torch.equal(run_min_dist(gpu, x, C, ref), phi)  # bitwise reproducible


@pytest.mark.parametrize("n", [1, 63, 4097, 100_003])
@pytest.mark.parametrize("ell", [0.5, 8, "10n"])
def test_sample_matches_spec(gpu, n, ell):
    from lua_mapreduce_1_amd.ops import kmeans as K
    ell = 10 * n if ell == "10n" else ell
    offset = 2 ** 33 + 5 if n == 4097 else 0
    X, C = blobs(n, 7, 3)
    x = torch.from_numpy(X).to(gpu)
    mind, _near, phi = K.min_dist(x, torch.from_numpy(C).to(gpu))
    idx, rows = K.sample(x, mind, phi, ell, 11, 2, offset=offset)
    widx, wrows = K.sample(torch.from_numpy(X), mind.cpu(), float(phi), ell, 11, 2, offset=offset)
    assert idx.dtype == torch.int64 and rows.dtype == torch.float32
    assert torch.equal(idx.cpu(), widx) and torch.equal(rows.cpu(), wrows)
    assert np.array_equal(rows.cpu().numpy(), X[idx.cpu().numpy() - offset])
    assert len(idx) <= n and (ell < 10 * n or len(idx) > n // 2)  # 10 n: all but the points far below the mean


def test_seed_job_gpu(gpu):
    from lua_mapreduce_1_amd.ops import kmeans as K
    m, _want = seed_job_checks(gpu, 20_000, 16, 8, GPU_JOB_SEED)
    info = m.SEED_INFO
    assert m.CENTROIDS.is_cuda
    assert np.array_equal(info["seeds"], K.recluster(info["candidates"], info["weights"], 8, GPU_JOB_SEED).numpy())
