// kmeans_seed.hip — the device half of k-means|| seeding (Bahmani et al.,
// "Scalable K-Means++"): a fused distance sweep that folds a batch of new
// candidates into every point's running nearest-candidate distance, and the
// Bernoulli D^2 sampling of the next batch with an ordered compaction and a
// fused row gather.  Self-contained, like kmeans.hip and kmeans_bf16.hip.
//
// mr_kmeans_min_dist.  X [n, d] fp32 or bf16, C [m, d] fp32 (this round's NEW
// candidates), mind fp32 [n], near int32 [n], base:
//
//   s_i    = min_j  ||c_j||^2 - 2 x_i . c_j        (fp32; lowest j on ties)
//   dist_i = max(0, fl(||x_i||^2) + s_i)
//   if dist_i < mind_i:  mind_i = dist_i, near_i = base + j*      (strict)
//   phi    = sum_i mind_i after the fold           (float64)
//
// 1 <= d <= 512, 1 <= m <= 16384, n >= 0.  bf16 points are widened exactly to
// fp32 while they are staged and run the fp32 MFMA path (there is no bf16-MFMA
// seeding path).  Non-finite coordinates are unspecified; near stays inside
// [base, base + m) or keeps its old value, nothing is indexed out of bounds.
//
// Work split.  Persistent workgroups of 4 waves; a workgroup owns a super-tile
// of 64 PT points, wave w the PT 16-point MFMA tiles at rows [16 PT w, ...).
// PT = 2 for d <= 64 and PT = 1 above, so that the tiles of d <= 128 take
// 67 584 bytes of LDS and TWO workgroups share a CU at every d <= 128 (there
// is no accumulation image here: all LDS goes to tiles).
//
//   * Points are staged in LDS coalesced along d (rows padded to a stride of
//     4 KS + 2 floats, the bank argument of kmeans.hip), ||x||^2 is taken per
//     point while its row is there, and each lane lifts its A fragments
//     a[tile][ks] = X[row = lane & 15][4 ks + (lane >> 4)] into registers for
//     the whole candidate sweep.  d > 128 runs in d-chunks of 128 with
//     accumulators that persist across the chunks (points re-staged per chunk).
//   * Candidates come in tiles of 64.  A thread holds its share of the NEXT
//     tile in registers (KS / 4 16-byte loads, issued before the current
//     tile's MFMA sweep, written to LDS after it): the sweep hides the global
//     latency that an accumulation phase would hide in the Lloyd step.
//     ||c||^2 is computed per staged tile (4 threads per candidate), +inf for
//     padding columns, which therefore never win.  m <= 64 and d <= 128: the
//     one tile is staged once per workgroup.
//   * f32-in MFMA on gfx950 is an exact k-ordered fma chain, so a score is
//     cn - 2 (length-d fma chain): the error bound of ops/kmeans.py.
//   * Epilogue: the 16 lanes of a row are reduced with xor-shuffles on (score,
//     index), the super-tile's scores, indices and ||x||^2 go to LDS, and the
//     first 64 PT threads do the global read-modify-write of mind and near as
//     one coalesced 4-byte stream per array.
//   * phi: every thread sums the folded mind of its points in float64; a
//     workgroup reduces in a fixed order into ITS slot of `partials`, and a
//     one-block launch sums the slots in a fixed order.  No float atomics: phi
//     is bitwise reproducible for equal inputs on one device.
//
// mr_kmeans_sample_count / mr_kmeans_sample_write.  Point i (global index
// g = offset + i) is selected iff phi != 0 and
//     float64(u24(seed, round, g)) * phi  <  ellp * float64(mind_i)
// (one IEEE multiply a side; ellp = ell 2^24 comes from the host), u24 the top
// 24 bits of h = F(F(F(F(seed + 0x9E3779B9) ^ round) ^ hi32(g)) ^ lo32(g)),
// F the murmur3 32-bit finaliser.  Three launches, no spinning, no look-back:
// count (a workgroup per 4096 points, 16-byte loads of mind), a one-block
// exclusive scan of the counts plus the total, and — after the host has read
// the total and sized the outputs — write: the rule again, ranks by wave ballot
// and popcount under per-(iteration, wave) LDS prefixes, so idx (int64, global
// indices) ascends, then the selected rows copied into rows[rank] coalesced
// along d (bf16 rows widened).
//
// Compiler resource report (gfx950, -O3, -Rpass-analysis=kernel-resource-usage;
// no scratch in any kernel; min_dist: fp32 / bf16 points, 32 static bytes of
// LDS plus the dynamic tiles listed):
//   kernel                         VGPRs      AGPRs  SGPRs  waves/SIMD  tile LDS (bytes)
//   min_dist KS = 4  PT 2 (d<=16)  134 / 136    32    106       3           15 616
//   min_dist KS = 16 PT 2 (d<=64)  206 / 206    32    106       2           52 480
//   min_dist KS = 32 PT 1 (d<=128) 228 / 228    16    106       2           67 584
//   min_dist KS = 32 PT 1 MULTI    203 / 203    16    106       2           67 584
//   phi                              9           0     15       8               32
//   sample count                    28           0     31       8               16
//   sample scan                     44           0     18       8            2 048
//   sample write                    28           0     42       8            8 452
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef float f32x2 __attribute__((ext_vector_type(2)));

namespace {

constexpr int SD_THREADS = 256;  // 4 waves
constexpr int SD_CT = 64;        // candidates per LDS tile (4 MFMA column tiles)
constexpr int SD_MAXD = 512, SD_MAXM = 16384;
constexpr int SD_LDS_MAX = 160 * 1024;
constexpr int SD_MAX_GROUPS = 2048;  // slots of `partials`
constexpr int SD_BLOCK = 4096;       // points per workgroup of the sampling launches

struct SdArgs {
  const void* X;  // fp32 or bf16 rows
  const float* C;
  float* mind;
  int* near;
  double* partials;
  long long n;
  int d, m, base;
  int vecx;  // d % 4 == 0 and X aligned for 4-element loads
  int vecc;  // d % 4 == 0 and C 16-byte aligned
};

__host__ __device__ constexpr int sd_stride(int ks) { return 4 * ks + 2; }
__host__ __device__ constexpr int sd_lds_floats(int ks, int pt) {
  return SD_CT * sd_stride(ks) + 64 * pt * sd_stride(ks) + SD_CT + 3 * 64 * pt;
}

__device__ __forceinline__ float sd_widen(uint16_t h) { return __uint_as_float((uint32_t)h << 16); }

// acc[s][t] += A_t (16 x 4KS) * B_s (4KS x 16); Cb = &Cs[first column tile][col][g]
template <int KS, int PT, int NS>
__device__ __forceinline__ void sd_mma(const float* __restrict__ Cb, const float (&a)[PT][KS], f32x4 (&acc)[NS][PT]) {
  constexpr int S = sd_stride(KS);
#pragma unroll
  for (int ks = 0; ks < KS; ++ks) {
#pragma unroll
    for (int s = 0; s < NS; ++s) {
      const float b = Cb[s * 16 * S + 4 * ks];
#pragma unroll
      for (int t = 0; t < PT; ++t) acc[s][t] = __builtin_amdgcn_mfma_f32_16x16x4f32(a[t][ks], b, acc[s][t], 0, 0, 0);
    }
  }
}

// running (best score, index) of the lane's rows; j0 = index of column tile 0's column
template <int PT, int NS>
__device__ __forceinline__ void sd_pick(const f32x4 (&acc)[NS][PT], const float* __restrict__ cnp, int j0,
                                        float (&best)[PT][4], int (&bidx)[PT][4]) {
#pragma unroll
  for (int s = 0; s < NS; ++s) {
    const float cn = cnp[s * 16];
#pragma unroll
    for (int t = 0; t < PT; ++t)
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

template <int KS, int PT, int NS>
__device__ __forceinline__ void sd_tile(const float* __restrict__ Cb, const float* __restrict__ cnp, int j0,
                                        const float (&a)[PT][KS], float (&best)[PT][4], int (&bidx)[PT][4]) {
  f32x4 acc[NS][PT];
#pragma unroll
  for (int s = 0; s < NS; ++s)
#pragma unroll
    for (int t = 0; t < PT; ++t) acc[s][t] = f32x4{0.f, 0.f, 0.f, 0.f};
  sd_mma<KS, PT, NS>(Cb, a, acc);
  sd_pick<PT, NS>(acc, cnp, j0, best, bidx);
}

// This thread's share of candidate rows [row0, row0 + 64) x columns [c0, c0 + 4 KS)
// into registers: element e = tid + 256 i covers row e / KS, columns 4 (e % KS) .. + 3.
// Every load is unconditional from a clamped (always valid) address; zero past either edge.
template <int KS>
__device__ __forceinline__ void sd_fetch(f32x4 (&pre)[KS / 4], const float* __restrict__ C, int row0, int m, int d,
                                         int c0, int vec, int tid) {
#pragma unroll
  for (int i = 0; i < KS / 4; ++i) {
    const int e = tid + SD_THREADS * i;
    const int r = row0 + e / KS, c = c0 + 4 * (e % KS);
    if (vec) {
      const bool ok = r < m && c < d;
      f32x4 v = *reinterpret_cast<const f32x4*>(C + (ok ? (size_t)r * d + c : (size_t)0));
      pre[i] = ok ? v : f32x4{0.f, 0.f, 0.f, 0.f};
    } else {
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        const bool ok = r < m && c + q < d;
        const float v = C[ok ? (size_t)r * d + c + q : (size_t)0];
        pre[i][q] = ok ? v : 0.f;
      }
    }
  }
}

template <int KS>
__device__ __forceinline__ void sd_put(float* __restrict__ Cs, const f32x4 (&pre)[KS / 4], int tid) {
  constexpr int S = sd_stride(KS);
#pragma unroll
  for (int i = 0; i < KS / 4; ++i) {
    const int e = tid + SD_THREADS * i;
    float* dst = Cs + (e / KS) * S + 4 * (e % KS);
    *reinterpret_cast<f32x2*>(dst) = f32x2{pre[i].x, pre[i].y};
    *reinterpret_cast<f32x2*>(dst + 2) = f32x2{pre[i].z, pre[i].w};
  }
}

// Stage point rows [row0, row0 + ROWS) x columns [c0, c0 + 4 KS) into LDS (row
// stride 4 KS + 2), zero past either edge, bf16 widened; loads as in sd_fetch.
template <int KS, int ROWS, bool BF16>
__device__ __forceinline__ void sd_stage(float* __restrict__ dst, const void* __restrict__ src, long long row0,
                                         long long nrows, int d, int c0, int vec, int tid) {
  constexpr int W = 4 * KS, S = sd_stride(KS);
  if (vec) {
    constexpr int W4 = W / 4;
#pragma unroll 8
    for (int e = tid; e < ROWS * W4; e += SD_THREADS) {
      const int r = e / W4, c = 4 * (e % W4);
      const bool ok = row0 + r < nrows && c0 + c < d;
      const size_t at = ok ? (size_t)(row0 + r) * d + c0 + c : (size_t)0;
      f32x4 v;
      if (BF16) {
        const uint2 h = *reinterpret_cast<const uint2*>((const uint16_t*)src + at);
        v = f32x4{__uint_as_float(h.x << 16), __uint_as_float(h.x & 0xFFFF0000u), __uint_as_float(h.y << 16),
                  __uint_as_float(h.y & 0xFFFF0000u)};
      } else {
        v = *reinterpret_cast<const f32x4*>((const float*)src + at);
      }
      if (!ok) v = f32x4{0.f, 0.f, 0.f, 0.f};
      *reinterpret_cast<f32x2*>(dst + r * S + c) = f32x2{v.x, v.y};
      *reinterpret_cast<f32x2*>(dst + r * S + c + 2) = f32x2{v.z, v.w};
    }
  } else {
#pragma unroll 8
    for (int e = tid; e < ROWS * W; e += SD_THREADS) {
      const int r = e / W, c = e % W;
      const bool ok = row0 + r < nrows && c0 + c < d;
      const size_t at = ok ? (size_t)(row0 + r) * d + c0 + c : (size_t)0;
      const float v = BF16 ? sd_widen(((const uint16_t*)src)[at]) : ((const float*)src)[at];
      dst[r * S + c] = ok ? v : 0.f;
    }
  }
}

// fixed-order sum of one double per thread over the workgroup; valid in thread 0
__device__ __forceinline__ double sd_block_sum(double v, double* red, int tid) {
#pragma unroll
  for (int m = 32; m >= 1; m >>= 1) v += __shfl_xor(v, m);
  if ((tid & 63) == 0) red[tid >> 6] = v;
  __syncthreads();
  return ((red[0] + red[1]) + red[2]) + red[3];
}

template <int KS, int PT, bool MULTI, bool BF16>
__global__ __launch_bounds__(SD_THREADS) void kmeans_min_dist_kernel(const SdArgs p) {
  constexpr int W = 4 * KS;  // floats of d per staged chunk
  constexpr int S = sd_stride(KS);
  constexpr int PW = 64 * PT;  // points per super-tile
  extern __shared__ float sd_lds[];
  __shared__ double red[4];
  float* Cs = sd_lds;                 // [SD_CT][S] candidate tile
  float* Xs = Cs + SD_CT * S;         // [PW][S]    point super-tile (chunk)
  float* cnS = Xs + PW * S;           // [SD_CT]    ||c||^2, +inf on padding
  float* xnS = cnS + SD_CT;           // [PW]       ||x||^2
  float* scS = xnS + PW;              // [PW]       winning score
  int* ixS = (int*)(scS + PW);        // [PW]       winning index

  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int col = lane & 15, g = lane >> 4;
  const int d = p.d, m = p.m;
  const long long n = p.n;
  const int nct = (m + SD_CT - 1) / SD_CT;
  const int nch = MULTI ? (d + W - 1) / W : 1;
  const long long nsuper = (n + PW - 1) / PW;
  const bool single = !MULTI && nct == 1;

  f32x4 pre[KS / 4];  // this thread's share of the next candidate tile
  sd_fetch<KS>(pre, p.C, 0, m, d, 0, p.vecc, tid);

  double myphi = 0.0;
  bool cstaged = false;
  for (long long st = blockIdx.x; st < nsuper; st += gridDim.x) {
    const long long base = st * PW;
    float a[PT][KS];
    float best[PT][4], xn[PT];
    int bidx[PT][4];
#pragma unroll
    for (int t = 0; t < PT; ++t) {
      xn[t] = 0.f;
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        best[t][i] = INFINITY;
        bidx[t][i] = 0;
      }
    }

    for (int ct = 0; ct < nct; ++ct) {
      f32x4 macc[4][PT];  // MULTI: the dot products across the d-chunks
      for (int dc = 0; dc < nch; ++dc) {
        const bool stage_c = !single || !cstaged;
        const bool stage_x = MULTI || ct == 0;
        __syncthreads();  // every reader of Cs / cnS / Xs / scS of the step before is done
        if (stage_c) sd_put<KS>(Cs, pre, tid);
        if (stage_x) sd_stage<KS, PW, BF16>(Xs, p.X, base, n, d, dc * W, p.vecx, tid);
        __syncthreads();
        if (stage_c) {  // ||c||^2 of the staged chunk: 4 threads per candidate
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
            cnS[r] = (ct * SD_CT + r < m) ? prev + s : INFINITY;
          }
          cstaged = true;
        }
        if (stage_x) {  // A fragments into registers (+ ||x||^2 on the first sweep)
#pragma unroll
          for (int t = 0; t < PT; ++t) {
            const float* xr = Xs + (wave * (16 * PT) + t * 16 + col) * S + g;
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
        if (!single) {  // the next step's tile: loads in flight behind the sweep below
          const bool wrap = dc + 1 == nch;
          const int nc = wrap ? (ct + 1 < nct ? ct + 1 : 0) : ct;
          sd_fetch<KS>(pre, p.C, nc * SD_CT, m, d, wrap ? 0 : (dc + 1) * W, p.vecc, tid);
        }
        __syncthreads();  // cnS visible
        const float* Cb = Cs + col * S + g;
        if (MULTI) {
          if (dc == 0) {
#pragma unroll
            for (int s = 0; s < 4; ++s)
#pragma unroll
              for (int t = 0; t < PT; ++t) macc[s][t] = f32x4{0.f, 0.f, 0.f, 0.f};
          }
          sd_mma<KS, PT, 4>(Cb, a, macc);
        } else {
          const int j0 = ct * SD_CT + col;
          const int nsub = min(4, (m - ct * SD_CT + 15) >> 4);
          if (nsub == 4) sd_tile<KS, PT, 4>(Cb, cnS + col, j0, a, best, bidx);
          else if (nsub == 3) sd_tile<KS, PT, 3>(Cb, cnS + col, j0, a, best, bidx);
          else if (nsub == 2) sd_tile<KS, PT, 2>(Cb, cnS + col, j0, a, best, bidx);
          else sd_tile<KS, PT, 1>(Cb, cnS + col, j0, a, best, bidx);
        }
      }
      if (MULTI) sd_pick<PT, 4>(macc, cnS + col, ct * SD_CT + col, best, bidx);
    }

    // the 16 lanes that share rows: (score, index) lexicographic minimum
#pragma unroll
    for (int t = 0; t < PT; ++t)
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        float s = best[t][i];
        int j = bidx[t][i];
#pragma unroll
        for (int mk = 8; mk >= 1; mk >>= 1) {
          const float os = __shfl_xor(s, mk);
          const int oj = __shfl_xor(j, mk);
          if (os < s || (os == s && oj < j)) {
            s = os;
            j = oj;
          }
        }
        if (col == 0) {
          const int q = wave * (16 * PT) + t * 16 + g * 4 + i;
          scS[q] = s;
          ixS[q] = min(max(j, 0), m - 1);
        }
      }
    if (g == 0) {
#pragma unroll
      for (int t = 0; t < PT; ++t) xnS[wave * (16 * PT) + t * 16 + col] = xn[t];
    }
    __syncthreads();

    if (tid < PW && base + tid < n) {  // the fold: one coalesced stream per array
      const float dist = fmaxf(0.f, xnS[tid] + scS[tid]);
      float cur = p.mind[base + tid];
      if (dist < cur) {
        cur = dist;
        p.mind[base + tid] = dist;
        p.near[base + tid] = p.base + ixS[tid];
      }
      myphi += (double)cur;
    }
  }

  const double s = sd_block_sum(myphi, red, tid);
  if (tid == 0) p.partials[blockIdx.x] = s;
}

__global__ __launch_bounds__(SD_THREADS) void kmeans_seed_phi_kernel(const double* __restrict__ partials, int nparts,
                                                                     double* __restrict__ phi) {
  __shared__ double red[4];
  double v = 0.0;
  for (int i = threadIdx.x; i < nparts; i += SD_THREADS) v += partials[i];
  const double s = sd_block_sum(v, red, threadIdx.x);
  if (threadIdx.x == 0) phi[0] = s;
}

// ---- sampling ----------------------------------------------------------------------

__host__ __device__ __forceinline__ uint32_t sd_fmix(uint32_t h) {  // murmur3's 32-bit finaliser
  h ^= h >> 16;
  h *= 0x85EBCA6Bu;
  h ^= h >> 13;
  h *= 0xC2B2AE35u;
  h ^= h >> 16;
  return h;
}

struct SdRule {
  double phi, ellp;
  uint32_t hs;  // F(F(seed + 0x9E3779B9) ^ round), from the host
  unsigned long long offset;
};

__device__ __forceinline__ bool sd_selected(const SdRule& r, long long i, float md) {
  const unsigned long long gi = r.offset + (unsigned long long)i;
  const uint32_t h = sd_fmix(sd_fmix(r.hs ^ (uint32_t)(gi >> 32)) ^ (uint32_t)gi);
  return r.phi != 0.0 && (double)(h >> 8) * r.phi < r.ellp * (double)md;
}

__global__ __launch_bounds__(SD_THREADS) void kmeans_sample_count_kernel(const float* __restrict__ mind, long long n,
                                                                         SdRule r, int vec,
                                                                         unsigned* __restrict__ counts) {
  __shared__ unsigned red[4];
  const int tid = threadIdx.x;
  const long long b0 = (long long)blockIdx.x * SD_BLOCK;
  unsigned c = 0;
#pragma unroll
  for (int it = 0; it < SD_BLOCK / (4 * SD_THREADS); ++it) {
    const long long i = b0 + it * 4 * SD_THREADS + 4 * tid;
    float v[4] = {0.f, 0.f, 0.f, 0.f};
    if (vec && i + 3 < n) {
      const f32x4 t = *reinterpret_cast<const f32x4*>(mind + i);
      v[0] = t.x, v[1] = t.y, v[2] = t.z, v[3] = t.w;
    } else {
#pragma unroll
      for (int q = 0; q < 4; ++q)
        if (i + q < n) v[q] = mind[i + q];
    }
#pragma unroll
    for (int q = 0; q < 4; ++q) c += (i + q < n && sd_selected(r, i + q, v[q])) ? 1u : 0u;
  }
#pragma unroll
  for (int m = 32; m >= 1; m >>= 1) c += __shfl_xor(c, m);
  if ((tid & 63) == 0) red[tid >> 6] = c;
  __syncthreads();
  if (tid == 0) counts[blockIdx.x] = red[0] + red[1] + red[2] + red[3];
}

// offs[b] = counts[0] + .. + counts[b - 1], total[0] = the sum of all: one workgroup
__global__ __launch_bounds__(SD_THREADS) void kmeans_sample_scan_kernel(const unsigned* __restrict__ counts,
                                                                        long long nb, long long* __restrict__ offs,
                                                                        long long* __restrict__ total) {
  __shared__ long long part[SD_THREADS];
  const int tid = threadIdx.x;
  const long long per = (nb + SD_THREADS - 1) / SD_THREADS;
  const long long lo = min(tid * per, nb), hi = min(lo + per, nb);
  long long s = 0;
  for (long long b = lo; b < hi; ++b) s += counts[b];
  part[tid] = s;
  __syncthreads();
  if (tid == 0) {
    long long run = 0;
    for (int t = 0; t < SD_THREADS; ++t) {
      const long long v = part[t];
      part[t] = run;
      run += v;
    }
    total[0] = run;
  }
  __syncthreads();
  long long run = part[tid];
  for (long long b = lo; b < hi; ++b) {
    offs[b] = run;
    run += counts[b];
  }
}

template <bool BF16>
__global__ __launch_bounds__(SD_THREADS) void kmeans_sample_write_kernel(const void* __restrict__ X,
                                                                         const float* __restrict__ mind, long long n,
                                                                         int d, SdRule r,
                                                                         const long long* __restrict__ offs,
                                                                         long long* __restrict__ idx,
                                                                         float* __restrict__ rows) {
  constexpr int ITS = SD_BLOCK / SD_THREADS;  // 16
  __shared__ unsigned wpre[ITS * 4];          // selected per (iteration, wave), then their exclusive prefixes
  __shared__ unsigned short sel[SD_BLOCK];    // block-local index of the rank-th selected point
  __shared__ unsigned cnt;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const long long b0 = (long long)blockIdx.x * SD_BLOCK;
  const long long out0 = offs[blockIdx.x];
  unsigned flags = 0;
#pragma unroll
  for (int it = 0; it < ITS; ++it) {
    const long long i = b0 + it * SD_THREADS + tid;
    const bool s = i < n && sd_selected(r, i, mind[i < n ? i : 0]);
    const unsigned long long bal = __ballot(s);
    if (lane == 0) wpre[it * 4 + wave] = (unsigned)__popcll(bal);
    flags |= (s ? 1u : 0u) << it;
  }
  __syncthreads();
  if (tid < 64) {  // exclusive prefixes in (iteration, wave) order: ascending point order
    const unsigned v = wpre[tid];
    unsigned x = v;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
      const unsigned t = __shfl_up(x, o);
      if (lane >= o) x += t;
    }
    wpre[tid] = x - v;
    if (tid == 63) cnt = x;
  }
  __syncthreads();
#pragma unroll
  for (int it = 0; it < ITS; ++it) {
    const bool s = (flags >> it) & 1u;
    const unsigned long long bal = __ballot(s);
    if (s) {
      const unsigned rk = wpre[it * 4 + wave] + (unsigned)__popcll(bal & ((1ull << lane) - 1ull));
      sel[rk] = (unsigned short)(it * SD_THREADS + tid);
      idx[out0 + rk] = (long long)(r.offset + (unsigned long long)(b0 + it * SD_THREADS + tid));
    }
  }
  __syncthreads();
  const int total = (int)cnt * d;  // <= 4096 * 512
  for (int e = tid; e < total; e += SD_THREADS) {  // the selected rows, coalesced along d
    const int rk = e / d, c = e - rk * d;
    const size_t at = (size_t)(b0 + sel[rk]) * d + c;
    rows[(size_t)(out0 + rk) * d + c] = BF16 ? sd_widen(((const uint16_t*)X)[at]) : ((const float*)X)[at];
  }
}

// ---- host side ---------------------------------------------------------------------

struct SdDevice {
  int lds = 0;  // LDS a workgroup may take (bytes)
  int cus = 0;
};

inline const SdDevice* sd_device() {
  static SdDevice devs[64];
  int dev = 0;
  if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= 64) return nullptr;
  SdDevice& D = devs[dev];
  if (D.cus == 0) {
    int lds = 0, cus = 0;
    if (hipDeviceGetAttribute(&lds, hipDeviceAttributeMaxSharedMemoryPerBlock, dev) != hipSuccess ||
        hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess || cus <= 0)
      return nullptr;
    D.lds = lds < SD_LDS_MAX ? lds : SD_LDS_MAX;
    D.cus = cus;
  }
  return &D;
}

// Launch one variant on a persistent grid: the workgroups the device holds at
// once (by the runtime's occupancy figure: registers and LDS), at most one per
// super-tile and at most SD_MAX_GROUPS.  Returns the grid, or < 0.
template <int KS, int PT, bool MULTI, bool BF16>
int sd_launch(const SdArgs& a, const SdDevice* D, hipStream_t s) {
  constexpr size_t lds = 4 * (size_t)sd_lds_floats(KS, PT);
  if (lds > (size_t)D->lds) return -3;
  static int occ = 0;  // workgroups per CU; the dynamic LDS above 64 KiB must be allowed once
  if (occ == 0) {
    // (the kernel's few static bytes come on top, so ask for the tiles, not for the device's whole LDS)
    if (hipFuncSetAttribute((const void*)kmeans_min_dist_kernel<KS, PT, MULTI, BF16>,
                            hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds) != hipSuccess) {
      (void)hipGetLastError();
      return -4;
    }
    int o = 0;
    if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&o, kmeans_min_dist_kernel<KS, PT, MULTI, BF16>, SD_THREADS,
                                                     lds) != hipSuccess)
      o = 0;
    (void)hipGetLastError();  // a failed query only costs the occupancy guess
    occ = o < 1 ? 1 : o > 4 ? 4 : o;
  }
  const long long nsuper = (a.n + 64 * PT - 1) / (64 * PT);
  long long grid = (long long)occ * D->cus;
  grid = grid > SD_MAX_GROUPS ? SD_MAX_GROUPS : grid;
  grid = grid > nsuper ? nsuper : grid;
  hipLaunchKernelGGL((kmeans_min_dist_kernel<KS, PT, MULTI, BF16>), dim3((unsigned)grid), dim3(SD_THREADS), lds, s, a);
  const int rc = (int)hipGetLastError();
  return rc ? -100 - rc : (int)grid;
}

template <bool BF16>
int sd_dispatch(const SdArgs& a, const SdDevice* D, hipStream_t s) {
  if (a.d > 128) return sd_launch<32, 1, true, BF16>(a, D, s);
  if (a.d > 64) return sd_launch<32, 1, false, BF16>(a, D, s);
  if (a.d > 16) return sd_launch<16, 2, false, BF16>(a, D, s);
  return sd_launch<4, 2, false, BF16>(a, D, s);
}

inline SdRule sd_rule(double phi, double ellp, unsigned seed, unsigned round, unsigned long long offset) {
  SdRule r;
  r.phi = phi;
  r.ellp = ellp;
  r.hs = sd_fmix(sd_fmix(seed + 0x9E3779B9u) ^ round);
  r.offset = offset;
  return r;
}

}  // namespace

extern "C" {

// float64 slots a min_dist call needs in `partials`
int mr_kmeans_seed_partials(void) { return SD_MAX_GROUPS; }

// Fold the candidates C [m, d] into mind / near and write phi (see the header).
// bf16 != 0: X holds bf16 rows.  partials: SD_MAX_GROUPS float64 of workspace.
// -2: shape outside 1 <= d <= 512, 1 <= m <= 16384, n >= 0;  -3: LDS too small;
// -4: the dynamic-LDS attribute was refused;  <= -100: -100 - the launch's HIP error.
int mr_kmeans_min_dist(const void* X, int bf16, const void* C, long long n, int d, int m, void* mind, void* near,
                       int base, void* partials, void* phi, hipStream_t s) {
  if (d < 1 || d > SD_MAXD || m < 1 || m > SD_MAXM || n < 0) return -2;
  int grid = 0;
  if (n > 0) {
    const SdDevice* D = sd_device();
    if (!D) return -1;
    SdArgs a;
    a.X = X;
    a.C = (const float*)C;
    a.mind = (float*)mind;
    a.near = (int*)near;
    a.partials = (double*)partials;
    a.n = n;
    a.d = d;
    a.m = m;
    a.base = base;
    a.vecx = (d % 4 == 0 && ((uintptr_t)X & (bf16 ? 7 : 15)) == 0) ? 1 : 0;
    a.vecc = (d % 4 == 0 && ((uintptr_t)C & 15) == 0) ? 1 : 0;
    grid = bf16 ? sd_dispatch<true>(a, D, s) : sd_dispatch<false>(a, D, s);
    if (grid < 0) return grid;
  }
  hipLaunchKernelGGL(kmeans_seed_phi_kernel, dim3(1), dim3(SD_THREADS), 0, s, (const double*)partials, grid,
                     (double*)phi);
  return (int)hipGetLastError();
}

// The count and scan launches of the sampling: counts uint32 [nb], offs int64
// [nb], total int64 [1], nb = ceil(n / 4096).
int mr_kmeans_sample_count(const void* mind, long long n, unsigned long long offset, double phi, double ellp,
                           unsigned seed, unsigned round, void* counts, void* offs, void* total, hipStream_t s) {
  if (n < 0) return -2;
  const long long nb = (n + SD_BLOCK - 1) / SD_BLOCK;
  if (nb > 0x7FFFFFFFll) return -2;
  const SdRule r = sd_rule(phi, ellp, seed, round, offset);
  if (nb > 0) {
    hipLaunchKernelGGL(kmeans_sample_count_kernel, dim3((unsigned)nb), dim3(SD_THREADS), 0, s, (const float*)mind, n,
                       r, ((uintptr_t)mind & 15) == 0 ? 1 : 0, (unsigned*)counts);
    const int rc = (int)hipGetLastError();
    if (rc) return rc;
  }
  hipLaunchKernelGGL(kmeans_sample_scan_kernel, dim3(1), dim3(SD_THREADS), 0, s, (const unsigned*)counts, nb,
                     (long long*)offs, (long long*)total);
  return (int)hipGetLastError();
}

// The write launch: idx int64 [total] and rows fp32 [total, d], from the same
// mind, rule arguments and offs that mr_kmeans_sample_count saw.
int mr_kmeans_sample_write(const void* X, int bf16, const void* mind, long long n, int d, unsigned long long offset,
                           double phi, double ellp, unsigned seed, unsigned round, const void* offs, void* idx,
                           void* rows, hipStream_t s) {
  if (n < 0 || d < 1 || d > SD_MAXD) return -2;
  const long long nb = (n + SD_BLOCK - 1) / SD_BLOCK;
  if (nb == 0) return 0;
  if (nb > 0x7FFFFFFFll) return -2;
  const SdRule r = sd_rule(phi, ellp, seed, round, offset);
  if (bf16)
    hipLaunchKernelGGL(kmeans_sample_write_kernel<true>, dim3((unsigned)nb), dim3(SD_THREADS), 0, s, X,
                       (const float*)mind, n, d, r, (const long long*)offs, (long long*)idx, (float*)rows);
  else
    hipLaunchKernelGGL(kmeans_sample_write_kernel<false>, dim3((unsigned)nb), dim3(SD_THREADS), 0, s, X,
                       (const float*)mind, n, d, r, (const long long*)offs, (long long*)idx, (float*)rows);
  return (int)hipGetLastError();
}

}  // extern "C"
