// kmeans.hip — the map step of Lloyd's k-means, fused: nearest-centroid
// assignment on the matrix cores and the per-cluster partial sums, in ONE
// launch.  The n x k distance matrix never exists, in HBM or anywhere else.
//
//   labels[i]  = argmin_j  ||c_j||^2 - 2 x_i . c_j          (lowest j on ties)
//   sums[j]   += sum of the x_i labelled j     (float64, added into)
//   counts[j] += their number                  (int64,   added into)
//   cost      += sum_i max(0, ||x_i||^2 + min_j score)      (float64, added into)
//
// X [n, d] and C [k, d] are fp32 row-major; 1 <= d <= 512, 1 <= k <= 4096.
// Non-finite coordinates are unspecified (a NaN score never wins a comparison,
// so such a point keeps some index in [0, k): the chosen index is clamped and
// nothing is ever indexed out of bounds).
//
// Work split.  A workgroup is 4 waves and owns a "super-tile" of 128 points:
// wave w owns two 16-point MFMA tiles (rows [32w, 32w+32)), the M dimension
// of __builtin_amdgcn_mfma_f32_16x16x4f32.  Workgroups are persistent: the
// grid is sized from the CU count and LDS use, and strides over super-tiles.
//
//   * The super-tile's points are staged in LDS (coalesced along d), then each
//     lane lifts its A fragments into registers: a[tile][ks] = X[row = lane&15]
//     [4 ks + (lane>>4)], KS = 4, 16 or 32 k-steps (d padded with zeros to 16,
//     64 or 128).  For d <= 128 they stay in registers for the whole centroid
//     sweep.  For d > 128 (MULTI) the points are re-staged in d-chunks of 128
//     per centroid tile and the accumulators persist across the chunks.
//   * Centroids stream through LDS in tiles of 64 (4 MFMA column tiles),
//     rows padded to a stride of 4 KS + 2 floats: a B-fragment read is
//     Cs[col][4 ks + g], bank (2 col + g + 4 ks) mod 32, distinct over the 32
//     lanes an LDS cycle serves (col 0..15, g in {0,1} or {2,3}).  One B read
//     feeds two MFMAs (the wave's two point tiles); a full centroid tile keeps
//     eight independent accumulator chains in flight.  The d and k tails are
//     zero in LDS; ||c_j||^2 is computed once per staged tile (4 threads per
//     centroid) and is +inf for padding centroids, so they never win.  With
//     k <= 64 and d <= 128 the one centroid tile is staged once per workgroup.
//   * f32-in MFMA on gfx950 is an exact k-ordered fma chain, so a score is the
//     fp32 value cn - 2 * (length-d fma chain): the error bound of the tests.
//   * Argmin in registers: C/D layout col = lane & 15, row = (lane>>4)*4 + reg,
//     so each lane keeps (best score, best index) for 2 x 4 rows across the
//     sweep — centroid indices reach a lane in ascending order and the compare
//     is strict, so the lowest index wins — then the 16 lanes of a row are
//     reduced with xor-shuffles on (score, index) lexicographically.
//   * Accumulation.  mode 1 (k (d + 1) floats fit the LDS left beside the
//     tiles): every point's row is added into an fp32 [k, d] image in LDS with
//     LDS atomics (2^lps lanes per point, coalesced along d), counts likewise;
//     ONE flush at the end of the workgroup adds the touched clusters to the
//     float64 / int64 global accumulators with native f64 / u64 atomics.
//     mode 2 (does not fit): each row goes straight to the global
//     accumulators, coalesced along d.  mode 0: labels (and cost) only.
//     The cost is summed per thread in float64 and added once per wave.
//
// No host synchronisation, no allocation, capture-safe (the dynamic-LDS
// attribute is a host-side function attribute set on first use).
//
// Compiler resource report (gfx950, -O3, -Rpass-analysis=kernel-resource-usage;
// no scratch in any variant; LDS is all dynamic: the tiles below, plus mode 1's
// 4 k (d + 1) bytes; the launcher takes up to the device's 160 KiB):
//   variant              VGPRs  AGPRs  SGPRs  waves/SIMD  tile LDS (bytes)
//   KS = 4  (d <= 16)     178     32    106       2            15 616
//   KS = 16 (d <= 64)     209     32    106       2            52 480
//   KS = 32 (d <= 128)    246     32    106       1           101 632
//   KS = 32 MULTI (> 128) 227     32    106       1           101 632
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

typedef float f32x4 __attribute__((ext_vector_type(4)));

namespace {

constexpr int KM_THREADS = 256;  // 4 waves
constexpr int KM_PT = 2;         // 16-point MFMA tiles per wave
constexpr int KM_PW = 4 * KM_PT * 16;  // points per workgroup super-tile (128)
constexpr int KM_CT = 64;        // centroids per LDS tile (4 MFMA column tiles)
constexpr int KM_MAXD = 512, KM_MAXK = 4096;
constexpr int KM_LDS_MAX = 160 * 1024;

struct KmArgs {
  const float* X;
  const float* C;
  double* sums;
  unsigned long long* counts;
  double* cost;
  int* labels;
  long long n;
  int d, k;
  int mode;  // 0 labels/cost only, 1 combine in LDS, 2 straight to global
  int lps;   // log2 of the lanes that share a point in the accumulation
  int vec;   // d % 4 == 0 and X, C 16-byte aligned: stage with 16-byte loads
};

__host__ __device__ constexpr int km_stride(int ks) { return 4 * ks + 2; }
__host__ __device__ constexpr int km_fixed_floats(int ks) {
  return KM_CT * km_stride(ks) + KM_PW * km_stride(ks) + KM_CT + 3 * KM_PW;
}

// acc[s][t] += A_t (16 x 4KS) * B_s (4KS x 16); Cb = &Cs[first column tile][col][g]
template <int KS, int NS>
__device__ __forceinline__ void km_mma(const float* __restrict__ Cb, const float (&a)[KM_PT][KS],
                                       f32x4 (&acc)[NS][KM_PT]) {
  constexpr int S = km_stride(KS);
#pragma unroll
  for (int ks = 0; ks < KS; ++ks) {
#pragma unroll
    for (int s = 0; s < NS; ++s) {
      const float b = Cb[s * 16 * S + 4 * ks];
#pragma unroll
      for (int t = 0; t < KM_PT; ++t) acc[s][t] = __builtin_amdgcn_mfma_f32_16x16x4f32(a[t][ks], b, acc[s][t], 0, 0, 0);
    }
  }
}

// running (best score, index) of the lane's rows; j0 = index of column tile 0's column
template <int NS>
__device__ __forceinline__ void km_pick(const f32x4 (&acc)[NS][KM_PT], const float* __restrict__ cnp, int j0,
                                        float (&best)[KM_PT][4], int (&bidx)[KM_PT][4]) {
#pragma unroll
  for (int s = 0; s < NS; ++s) {
    const float cn = cnp[s * 16];
#pragma unroll
    for (int t = 0; t < KM_PT; ++t)
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const float sc = fmaf(-2.f, acc[s][t][i], cn);
        if (sc < best[t][i]) {
          best[t][i] = sc;
          bidx[t][i] = j0 + s * 16;
        }
      }
  }
}

template <int KS, int NS>
__device__ __forceinline__ void km_tile(const float* __restrict__ Cb, const float* __restrict__ cnp, int j0,
                                        const float (&a)[KM_PT][KS], float (&best)[KM_PT][4],
                                        int (&bidx)[KM_PT][4]) {
  f32x4 acc[NS][KM_PT];
#pragma unroll
  for (int s = 0; s < NS; ++s)
#pragma unroll
    for (int t = 0; t < KM_PT; ++t) acc[s][t] = f32x4{0.f, 0.f, 0.f, 0.f};
  km_mma<KS, NS>(Cb, a, acc);
  km_pick<NS>(acc, cnp, j0, best, bidx);
}

// Stage rows [row0, row0 + ROWS) x columns [c0, c0 + 4 KS) of a row-major [nrows, d]
// matrix into LDS (row stride 4 KS + 2), zero past either edge.  Every load is
// unconditional from a clamped (always valid) address and the loops unroll,
// so a thread keeps many loads in flight; 16-byte loads when d % 4 == 0 and
// the base is aligned (vec).
template <int KS, int ROWS>
__device__ __forceinline__ void km_stage(float* __restrict__ dst, const float* __restrict__ src, long long row0,
                                         long long nrows, int d, int c0, int vec, int tid) {
  constexpr int W = 4 * KS, S = km_stride(KS);
  typedef float f32x2 __attribute__((ext_vector_type(2)));
  if (vec) {
    constexpr int W4 = W / 4;
#pragma unroll 8
    for (int e = tid; e < ROWS * W4; e += KM_THREADS) {
      const int r = e / W4, c = 4 * (e % W4);
      const bool ok = row0 + r < nrows && c0 + c < d;
      f32x4 v = *reinterpret_cast<const f32x4*>(src + (ok ? (size_t)(row0 + r) * d + c0 + c : (size_t)0));
      if (!ok) v = f32x4{0.f, 0.f, 0.f, 0.f};
      *reinterpret_cast<f32x2*>(dst + r * S + c) = f32x2{v.x, v.y};
      *reinterpret_cast<f32x2*>(dst + r * S + c + 2) = f32x2{v.z, v.w};
    }
  } else {
#pragma unroll 8
    for (int e = tid; e < ROWS * W; e += KM_THREADS) {
      const int r = e / W, c = e % W;
      const bool ok = row0 + r < nrows && c0 + c < d;
      const float v = src[ok ? (size_t)(row0 + r) * d + c0 + c : (size_t)0];
      dst[r * S + c] = ok ? v : 0.f;
    }
  }
}

template <int KS, bool MULTI>
__global__ __launch_bounds__(KM_THREADS) void kmeans_step_kernel(const KmArgs p) {
  constexpr int W = 4 * KS;  // floats of d per staged chunk
  constexpr int S = km_stride(KS);
  extern __shared__ float km_lds[];
  float* Cs = km_lds;                       // [KM_CT][S] centroid tile
  float* Xs = Cs + KM_CT * S;               // [KM_PW][S] point super-tile (chunk)
  float* cnS = Xs + KM_PW * S;              // [KM_CT]   ||c||^2, +inf on padding
  float* xnS = cnS + KM_CT;                 // [KM_PW]   ||x||^2
  float* bestS = xnS + KM_PW;               // [KM_PW]   winning score
  int* labS = (int*)(bestS + KM_PW);        // [KM_PW]   winning index
  float* ls = (float*)(labS + KM_PW);       // [k][d]    mode 1: fp32 partial sums
  unsigned* lc = (unsigned*)(ls + (size_t)p.k * p.d);  // [k] mode 1: counts

  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int col = lane & 15, g = lane >> 4;
  const int d = p.d, k = p.k;
  const long long n = p.n;
  const int nct = (k + KM_CT - 1) / KM_CT;
  const int nch = MULTI ? (d + W - 1) / W : 1;
  const long long nsuper = (n + KM_PW - 1) / KM_PW;

  if (p.mode == 1) {
    for (int e = tid; e < k * d; e += KM_THREADS) ls[e] = 0.f;
    for (int e = tid; e < k; e += KM_THREADS) lc[e] = 0u;
  }

  double mycost = 0.0;
  bool cstaged = false;
  for (long long st = blockIdx.x; st < nsuper; st += gridDim.x) {
    const long long base = st * KM_PW;
    float a[KM_PT][KS];
    float best[KM_PT][4], xn[KM_PT];
    int bidx[KM_PT][4];
#pragma unroll
    for (int t = 0; t < KM_PT; ++t) {
      xn[t] = 0.f;
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        best[t][i] = INFINITY;
        bidx[t][i] = 0;
      }
    }

    for (int ct = 0; ct < nct; ++ct) {
      f32x4 macc[4][KM_PT];  // MULTI: scores' dot products across the d-chunks
      for (int dc = 0; dc < nch; ++dc) {
        const bool stage_c = MULTI || nct > 1 || !cstaged;
        const bool stage_x = MULTI || ct == 0;
        const int c0 = dc * W;
        __syncthreads();  // every reader of Cs / cnS / Xs / labS of the step before is done
        if (stage_c) km_stage<KS, KM_CT>(Cs, p.C, (long long)ct * KM_CT, k, d, c0, p.vec, tid);
        if (stage_x) km_stage<KS, KM_PW>(Xs, p.X, base, n, d, c0, p.vec, tid);
        __syncthreads();
        if (stage_c) {  // ||c||^2 of the staged chunk: 4 threads per centroid
          const int r = tid >> 2, q = tid & 3;
          float s = 0.f;
#pragma unroll 8
          for (int i = 0; i < KS; ++i) {
            const float v = Cs[r * S + 4 * i + q];
            s = fmaf(v, v, s);
          }
          s += __shfl_xor(s, 1);
          s += __shfl_xor(s, 2);
          if (q == 0) {
            const float prev = (MULTI && dc > 0) ? cnS[r] : 0.f;
            cnS[r] = (ct * KM_CT + r < k) ? prev + s : INFINITY;
          }
          cstaged = true;
        }
        if (stage_x) {  // A fragments into registers (+ ||x||^2 on the first sweep)
#pragma unroll
          for (int t = 0; t < KM_PT; ++t) {
            const float* xr = Xs + (wave * (16 * KM_PT) + t * 16 + col) * S + g;
            float s = 0.f;
#pragma unroll
            for (int ks = 0; ks < KS; ++ks) {
              a[t][ks] = xr[4 * ks];
              s = fmaf(a[t][ks], a[t][ks], s);
            }
            if (ct == 0) {
              s += __shfl_xor(s, 16);
              s += __shfl_xor(s, 32);
              xn[t] += s;
            }
          }
        }
        __syncthreads();  // cnS visible
        const float* Cb = Cs + col * S + g;
        if (MULTI) {
          if (dc == 0) {
#pragma unroll
            for (int s = 0; s < 4; ++s)
#pragma unroll
              for (int t = 0; t < KM_PT; ++t) macc[s][t] = f32x4{0.f, 0.f, 0.f, 0.f};
          }
          km_mma<KS, 4>(Cb, a, macc);
        } else {
          const int j0 = ct * KM_CT + col;
          const int nsub = min(4, (k - ct * KM_CT + 15) >> 4);
          if (nsub == 4) km_tile<KS, 4>(Cb, cnS + col, j0, a, best, bidx);
          else if (nsub == 3) km_tile<KS, 3>(Cb, cnS + col, j0, a, best, bidx);
          else if (nsub == 2) km_tile<KS, 2>(Cb, cnS + col, j0, a, best, bidx);
          else km_tile<KS, 1>(Cb, cnS + col, j0, a, best, bidx);
        }
      }
      if (MULTI) km_pick<4>(macc, cnS + col, ct * KM_CT + col, best, bidx);
    }

    // the 16 lanes that share rows: (score, index) lexicographic minimum
#pragma unroll
    for (int t = 0; t < KM_PT; ++t)
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        float s = best[t][i];
        int j = bidx[t][i];
#pragma unroll
        for (int m = 8; m >= 1; m >>= 1) {
          const float os = __shfl_xor(s, m);
          const int oj = __shfl_xor(j, m);
          if (os < s || (os == s && oj < j)) {
            s = os;
            j = oj;
          }
        }
        if (col == 0) {
          const int q = wave * (16 * KM_PT) + t * 16 + g * 4 + i;
          j = min(max(j, 0), k - 1);
          labS[q] = j;
          bestS[q] = s;
          if (p.labels && base + q < n) p.labels[base + q] = j;
        }
      }
    if (g == 0) {
#pragma unroll
      for (int t = 0; t < KM_PT; ++t) xnS[wave * (16 * KM_PT) + t * 16 + col] = xn[t];
    }
    __syncthreads();

    if (tid < KM_PW && base + tid < n) mycost += (double)fmaxf(0.f, xnS[tid] + bestS[tid]);

    if (p.mode != 0) {  // add the rows into their clusters: 2^lps lanes per point, along d
      const int lp = 1 << p.lps, ppi = 64 >> p.lps;
      const int cl = lane & (lp - 1);
      for (int q = wave * ppi + (lane >> p.lps); q < KM_PW; q += 4 * ppi) {
        const long long i = base + q;
        if (i >= n) continue;
        const int L = labS[q];
        if (p.mode == 1) {
          for (int c = cl; c < d; c += lp) {
            const float x = MULTI ? p.X[(size_t)i * d + c] : Xs[q * S + c];
            atomicAdd(&ls[L * d + c], x);
          }
          if (cl == 0) atomicAdd(&lc[L], 1u);
        } else {
          if (p.sums)
            for (int c = cl; c < d; c += lp) {
              const float x = MULTI ? p.X[(size_t)i * d + c] : Xs[q * S + c];
              unsafeAtomicAdd(&p.sums[(size_t)L * d + c], (double)x);
            }
          if (cl == 0 && p.counts) atomicAdd(&p.counts[L], 1ull);
        }
      }
    }
  }

  if (p.cost) {
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) mycost += __shfl_xor(mycost, m);
    if (lane == 0 && mycost != 0.0) unsafeAtomicAdd(p.cost, mycost);
  }
  if (p.mode == 1) {  // the one flush: touched clusters only
    __syncthreads();
    if (p.sums)
      for (int e = tid; e < k * d; e += KM_THREADS)
        if (lc[e / d]) unsafeAtomicAdd(&p.sums[e], (double)ls[e]);
    if (p.counts)
      for (int j = tid; j < k; j += KM_THREADS)
        if (lc[j]) atomicAdd(&p.counts[j], (unsigned long long)lc[j]);
  }
}

// k-steps of the variant that serves d, and whether it chunks d
inline int km_ksteps(int d) { return d <= 16 ? 4 : d <= 64 ? 16 : 32; }

struct KmDevice {
  int lds = 0;  // LDS a workgroup may take (bytes)
  int cus = 0;
};

inline const KmDevice* km_device() {
  static KmDevice devs[64];
  int dev = 0;
  if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= 64) return nullptr;
  KmDevice& D = devs[dev];
  if (D.cus == 0) {
    int lds = 0, cus = 0;
    if (hipDeviceGetAttribute(&lds, hipDeviceAttributeMaxSharedMemoryPerBlock, dev) != hipSuccess ||
        hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess || cus <= 0)
      return nullptr;
    D.lds = lds < KM_LDS_MAX ? lds : KM_LDS_MAX;
    D.cus = cus;
  }
  return &D;
}

// largest k whose [k, d] fp32 partial sums and k counts fit beside the tiles
inline int km_lds_limit(int d, int lds) {
  const long long left = (long long)lds - 4ll * km_fixed_floats(km_ksteps(d));
  return left <= 0 ? 0 : (int)(left / (4ll * (d + 1)));
}

template <int KS, bool MULTI>
int km_launch(const KmArgs& a, size_t lds, unsigned grid, hipStream_t s) {
  static bool lds_attr = false;  // dynamic LDS above 64 KiB must be allowed once
  if (!lds_attr) {
    (void)hipFuncSetAttribute((const void*)kmeans_step_kernel<KS, MULTI>, hipFuncAttributeMaxDynamicSharedMemorySize,
                              KM_LDS_MAX);
    lds_attr = true;
  }
  hipLaunchKernelGGL((kmeans_step_kernel<KS, MULTI>), dim3(grid), dim3(KM_THREADS), lds, s, a);
  return (int)hipGetLastError();
}

}  // namespace

extern "C" {

// Largest k for which a step at this d combines its sums in LDS (mode 1); a
// larger k adds straight to the global accumulators (mode 2).  < 0: no device.
int mr_kmeans_lds_limit(int d) {
  if (d < 1 || d > KM_MAXD) return -2;
  const KmDevice* D = km_device();
  return D ? km_lds_limit(d, D->lds) : -1;
}

// One k-means map step (see the header).  sums / counts / cost are added into
// and may each be null; labels may be null.  -2: shape outside 1 <= d <= 512,
// 1 <= k <= 4096, n >= 0;  -3: the device's LDS cannot hold the tiles.
int mr_kmeans_step(const void* X, const void* C, long long n, int d, int k, void* sums, void* counts, void* cost,
                   void* labels, hipStream_t s) {
  if (d < 1 || d > KM_MAXD || k < 1 || k > KM_MAXK || n < 0) return -2;
  if (n == 0) return 0;
  const KmDevice* D = km_device();
  if (!D) return -1;
  const int ks = km_ksteps(d);
  size_t lds = 4 * (size_t)km_fixed_floats(ks);
  if (lds > (size_t)D->lds) return -3;
  KmArgs a;
  a.X = (const float*)X;
  a.C = (const float*)C;
  a.sums = (double*)sums;
  a.counts = (unsigned long long*)counts;
  a.cost = (double*)cost;
  a.labels = (int*)labels;
  a.n = n;
  a.d = d;
  a.k = k;
  a.mode = (!sums && !counts) ? 0 : (k <= km_lds_limit(d, D->lds) ? 1 : 2);
  if (a.mode == 1) lds += 4 * (size_t)k * (d + 1);
  a.lps = 0;
  while (a.lps < 6 && (1 << a.lps) < d) ++a.lps;
  a.vec = (d % 4 == 0 && (((uintptr_t)X | (uintptr_t)C) & 15) == 0) ? 1 : 0;
  const long long nsuper = (n + KM_PW - 1) / KM_PW;
  long long wpc = KM_LDS_MAX / (long long)lds;
  wpc = wpc < 1 ? 1 : wpc > 4 ? 4 : wpc;
  const unsigned grid = (unsigned)(nsuper < wpc * D->cus ? nsuper : wpc * D->cus);
  if (d > 128) return km_launch<32, true>(a, lds, grid, s);
  if (ks == 32) return km_launch<32, false>(a, lds, grid, s);
  if (ks == 16) return km_launch<16, false>(a, lds, grid, s);
  return km_launch<4, false>(a, lds, grid, s);
}

}  // extern "C"
