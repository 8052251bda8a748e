// gmm.hip — one EM step of a diagonal-covariance Gaussian mixture, fused on the
// fp32 matrix cores.  The n x k score / responsibility matrix never exists in
// HBM: it is produced in registers by one MFMA product and consumed, still in
// registers, as the left operand of a second one.
//
//   A[j, c] = mu_jc / var_jc,  A[j, d + c] = -1/2 / var_jc            (fp32 [k, 2d])
//   b[j]    = log w_j - 1/2 sum_c (log(2 pi var_jc) + mu_jc^2 / var_jc)   (fp32 [k])
//   s_ij    = b_j + sum_c A[j, c] x_ic + sum_c A[j, d + c] x_ic^2
//   logp_i  = log sum_j exp s_ij          labels_i = argmax_j s_ij (lowest j on ties)
//   r_ij    = exp(s_ij - logp_i)
//   nk[j] += sum_i r_ij   s1[j, c] += sum_i r_ij x_ic   s2[j, c] += sum_i r_ij x_ic^2
//   ll    += sum_i logp_i                                   (all float64, added into)
//
// X [n, d] fp32 row-major, 1 <= d <= 128, 1 <= k <= 4096.  Three launches.
//
// 1. gmm_prepare_kernel (one wave per component).  A's entries are the float64
//    quotient rounded once to fp32; b is summed in float64 and rounded once.
//    Both passes below read the A, b this launch wrote and nothing else of the
//    parameters.
//
// 2. gmm_score_kernel (pass 1), the plan of kmeans.hip: persistent 4-wave
//    workgroups own 128-point super-tiles, wave w the rows [32w, 32w + 32) as
//    two 16-point MFMA tiles.  The points are staged in LDS (row stride
//    4 KS + 2) and each lane lifts a[t][ks] = X[row = lane & 15][4 ks + (lane >>
//    4)] into registers for the whole sweep.  The x^2 half of the augmented row
//    is never stored: a * a is formed in fp32 (one rounding) right before the
//    MFMA that consumes it, one v_mul per NS MFMAs.  A streams through LDS in
//    tiles of 64 components, its two halves as two [64][4 KS + 2] images; a B
//    read is As[col][4 ks + g], bank (2 col + g + 4 ks) mod 32, distinct over
//    the 32 lanes of an LDS cycle.  A score is b_j + (an exact k-ordered fp32
//    fma chain of length 2d, x and x^2 terms interleaved in steps of four).
//    Each lane keeps, for its 2 x 4 rows, the ONLINE triple (running max m,
//    running l = sum exp(s - m), index of the max): per component tile the new
//    max is taken first, l is rescaled once by exp(m_old - m_new) and the
//    tile's NS terms are added.  m = -inf (nothing but padding seen so far) is
//    replaced by 0 inside the exponents only, so exp(-inf - (-inf)) never
//    occurs; padding components have b = -inf and add exp(-inf) = 0.  Indices
//    reach a lane in ascending order and the compare is strict, so the lowest
//    index keeps a tie; the 16 lanes of a row are merged with xor-shuffles.
//    logp = m + logf(l).  ll: float64 per thread, one f64 atomic per wave.
//
// 3. gmm_stats_kernel (pass 2).  Grid = (slab of points) x (component tile of
//    16 NS <= 64; <= 32 for d > 64).  The workgroup stages its A tile once,
//    then per 128-point super-tile of its slab: stages the points (row stride 4 KS + 4) and their
//    logp (+inf for rows past n, so r = 0), lifts the fragments, recomputes the
//    128 x 16NS score block with the first product — the same chain as pass 1,
//    so the same bits — and turns it into r = expf((acc + b) - logp) in place.
//    How r reaches the A operand of the second product: it does not move.  In
//    the 16x16x4 accumulator layout lane (col, g) holds rows 4g .. 4g + 3 of
//    column col, i.e. r[point 4g + i][component col].  An A operand wants
//    A[M = lane & 15][K = lane >> 4]; with M = component and K = point,
//    register i of the accumulator IS the A operand of a k-step that contracts
//    over the points {i, 4 + i, 8 + i, 12 + i} of the tile.  The B operand of
//    that k-step is B[K = g][N = col] = Xs[point 4g + i][16 c + col], read in
//    the same permuted order, and its square (again formed on the fly) for the
//    x^2 columns.  No transpose, no LDS round trip, no cross-lane traffic.
//    LDS banks of that read: address (p0 + 4g + i) SX + 16c + col with SX =
//    4 KS + 4, so the two g of an LDS cycle differ by 4 SX = 16 (mod 32) and
//    the 16 col are consecutive: 32 distinct banks.  (The price: the fragment
//    lift Xs[row SX + 4 ks + g] with SX = 4 (mod 32) puts rows r and r + 8 on
//    one bank, a 2-way conflict on 2 KS reads per wave and super-tile, against
//    8 KS/4 + 2 KS NS conflict-free ones.)  Every wave keeps the full
//    [16 NS] x [X | X^2] accumulator block for its own 32 rows of each
//    super-tile: 2 NS (KS / 4) f32x4, which the compiler places in AGPRs.  nk
//    needs no ones column: r is summed per lane and folded over g at the end.
//    A slab is at most RUN = 4096 points, so no fp32 accumulator ever holds
//    more than RUN terms.  At the end of the slab the four waves fold their
//    blocks into one fp32 image in LDS (over the dead A / X tiles), and the
//    workgroup adds the image's live, non-zero entries, widened to float64,
//    into nk / s1 / s2 with native f64 atomics.  Slabs are sized from the CU
//    count: about four workgroups per CU at any k, never more than RUN points.
//
// No host synchronisation, no allocation, no memset: capture-safe (the dynamic-
// LDS attribute is a host-side function attribute set on first use).
//
// Compiler resource report (gfx950, -O3, packed fp32 ops off,
// -Rpass-analysis=kernel-resource-usage; no scratch in any variant; LDS is all
// dynamic):
//   kernel                 VGPRs  AGPRs  SGPRs  waves/SIMD  LDS (bytes)
//   gmm_prepare_kernel        62      0     36       8              0
//   score KS = 4  (d <= 16)  215     48    106       1         19 200
//   score KS = 16 (d <= 64)  234     48    106       1         68 352
//   score KS = 32 (d <= 128) 256     71    106       1        133 888
//   stats KS = 4,  NS = 1     89     16     59       4         13 120
//   stats KS = 4,  NS = 2     97     24     59       4         15 488
//   stats KS = 4,  NS = 3    120     48     60       3         17 856
//   stats KS = 4,  NS = 4    132     64     62       2         20 224
//   stats KS = 16, NS = 1    103     48     82       3         43 840
//   stats KS = 16, NS = 2    112     92     82       2         52 352
//   stats KS = 16, NS = 3    128    132     82       1         60 864
//   stats KS = 16, NS = 4    161    172     84       1         69 376
//   stats KS = 32, NS = 1     95     80     80       2         84 800
//   stats KS = 32, NS = 2    161    156     80       1        101 504
// (NS = 16-component column tiles of the statistics pass's component tile:
// min(4, ceil(k / 16)), at most 2 for d > 64, where a 64-component block of
// accumulators alone would take 256 registers and the compiler spills.  The
// score kernel's AGPRs at KS = 32 hold VGPR copies, not scratch.)
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef float f32x2 __attribute__((ext_vector_type(2)));

namespace {

constexpr int GM_THREADS = 256;  // 4 waves
constexpr int GM_PT = 2;         // 16-point MFMA tiles per wave
constexpr int GM_PW = 128;       // points per super-tile
constexpr int GM_CT = 64;        // components per LDS tile of pass 1
constexpr int GM_MAXD = 128, GM_MAXK = 4096;
constexpr int GM_RUN = 4096;     // most points an fp32 accumulator of pass 2 sums
constexpr int GM_LDS_MAX = 160 * 1024;

__device__ __forceinline__ void gm_mfma(float a, float b, f32x4& c) {
  c = __builtin_amdgcn_mfma_f32_16x16x4f32(a, b, c, 0, 0, 0);
}

// Stage rows [row0, row0 + ROWS) x columns [c0, c0 + W) of a row-major matrix
// with leading dimension ld into LDS (row stride S), zero past row nrows or
// column c0 + cols.  Loads are unconditional from a clamped address.
template <int W, int S, int ROWS>
__device__ __forceinline__ void gm_stage(float* __restrict__ dst, const float* __restrict__ src, long long row0,
                                         long long nrows, int ld, int c0, int cols, int vec, int tid) {
  if (vec) {
    constexpr int W4 = W / 4;
#pragma unroll 8
    for (int e = tid; e < ROWS * W4; e += GM_THREADS) {
      const int r = e / W4, c = 4 * (e % W4);
      const bool ok = row0 + r < nrows && c < cols;
      f32x4 v = *reinterpret_cast<const f32x4*>(src + (ok ? (size_t)(row0 + r) * ld + c0 + c : (size_t)0));
      if (!ok) v = f32x4{0.f, 0.f, 0.f, 0.f};
      *reinterpret_cast<f32x2*>(dst + r * S + c) = f32x2{v.x, v.y};
      *reinterpret_cast<f32x2*>(dst + r * S + c + 2) = f32x2{v.z, v.w};
    }
  } else {
#pragma unroll 8
    for (int e = tid; e < ROWS * W; e += GM_THREADS) {
      const int r = e / W, c = e % W;
      const bool ok = row0 + r < nrows && c < cols;
      const float v = src[ok ? (size_t)(row0 + r) * ld + c0 + c : (size_t)0];
      dst[r * S + c] = ok ? v : 0.f;
    }
  }
}

// acc[s][t] = the length-2d chains of point tile t against column tile s.
// Ab = &As[0][col][g]; the x^2 half of A lies HALF floats further.
template <int KS, int NS, int S, int HALF>
__device__ __forceinline__ void gm_scores(const float* __restrict__ Ab, const float (&a)[GM_PT][KS],
                                          f32x4 (&acc)[NS][GM_PT]) {
#pragma unroll
  for (int s = 0; s < NS; ++s)
#pragma unroll
    for (int t = 0; t < GM_PT; ++t) acc[s][t] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
  for (int ks = 0; ks < KS; ++ks) {
    float b1[NS], b2[NS], a2[GM_PT];
#pragma unroll
    for (int s = 0; s < NS; ++s) {
      b1[s] = Ab[s * 16 * S + 4 * ks];
      b2[s] = Ab[HALF + s * 16 * S + 4 * ks];
    }
#pragma unroll
    for (int t = 0; t < GM_PT; ++t) a2[t] = a[t][ks] * a[t][ks];
#pragma unroll
    for (int s = 0; s < NS; ++s)
#pragma unroll
      for (int t = 0; t < GM_PT; ++t) gm_mfma(a[t][ks], b1[s], acc[s][t]);
#pragma unroll
    for (int s = 0; s < NS; ++s)
#pragma unroll
      for (int t = 0; t < GM_PT; ++t) gm_mfma(a2[t], b2[s], acc[s][t]);
  }
}

// ---- prepare -------------------------------------------------------------------------------

__global__ __launch_bounds__(64) void gmm_prepare_kernel(const float* __restrict__ w, const float* __restrict__ M,
                                                         const float* __restrict__ V, int d, int k,
                                                         float* __restrict__ A, float* __restrict__ b) {
  const int j = blockIdx.x, lane = threadIdx.x;
  if (j >= k) return;
  double acc = 0.0;
  for (int c = lane; c < d; c += 64) {
    const double mu = (double)M[(size_t)j * d + c], var = (double)V[(size_t)j * d + c];
    A[(size_t)j * 2 * d + c] = (float)(mu / var);
    A[(size_t)j * 2 * d + d + c] = (float)(-0.5 / var);
    acc += log(6.283185307179586 * var) + mu * mu / var;
  }
#pragma unroll
  for (int m = 32; m >= 1; m >>= 1) acc += __shfl_xor(acc, m);
  if (lane == 0) b[j] = (float)(log((double)w[j]) - 0.5 * acc);
}

// ---- pass 1: scores, online log-sum-exp, arg-max -------------------------------------------

struct GmScoreArgs {
  const float* X;
  const float* A;
  const float* b;
  float* logp;
  int* labels;
  double* ll;
  long long n;
  int d, k;
  int vec;  // d % 4 == 0 and X, A 16-byte aligned: stage with 16-byte loads
};

__host__ __device__ constexpr int gm_score_floats(int ks) {
  return 2 * GM_CT * (4 * ks + 2) + GM_PW * (4 * ks + 2) + GM_CT + GM_PW;
}

template <int KS, int NS>
__device__ __forceinline__ void gm_online(const float* __restrict__ Ab, const float* __restrict__ bp, int j0,
                                          const float (&a)[GM_PT][KS], float (&m)[GM_PT][4], float (&l)[GM_PT][4],
                                          int (&bidx)[GM_PT][4]) {
  constexpr int S = 4 * KS + 2;
  f32x4 acc[NS][GM_PT];
  gm_scores<KS, NS, S, GM_CT * S>(Ab, a, acc);
  float bj[NS];
#pragma unroll
  for (int s = 0; s < NS; ++s) bj[s] = bp[s * 16];
#pragma unroll
  for (int t = 0; t < GM_PT; ++t)
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      float sc[NS], mn = m[t][i];
#pragma unroll
      for (int s = 0; s < NS; ++s) {
        sc[s] = acc[s][t][i] + bj[s];
        if (sc[s] > mn) {
          mn = sc[s];
          bidx[t][i] = j0 + s * 16;
        }
      }
      const float ms = mn == -INFINITY ? 0.f : mn;
      float sum = l[t][i] * expf(m[t][i] - ms);
#pragma unroll
      for (int s = 0; s < NS; ++s) sum += expf(sc[s] - ms);
      l[t][i] = sum;
      m[t][i] = mn;
    }
}

template <int KS>
__global__ __launch_bounds__(GM_THREADS) void gmm_score_kernel(const GmScoreArgs p) {
  constexpr int W = 4 * KS, S = W + 2;
  extern __shared__ float gm_lds[];
  float* As = gm_lds;              // [2][GM_CT][S]  the x half, then the x^2 half
  float* Xs = As + 2 * GM_CT * S;  // [GM_PW][S]
  float* bS = Xs + GM_PW * S;      // [GM_CT]  b, -inf on padding
  float* lpS = bS + GM_CT;         // [GM_PW]  logp of the super-tile

  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int col = lane & 15, g = lane >> 4;
  const int d = p.d, k = p.k;
  const long long n = p.n;
  const int nct = (k + GM_CT - 1) / GM_CT;
  const long long nsuper = (n + GM_PW - 1) / GM_PW;

  double myll = 0.0;
  bool astaged = false;
  for (long long st = blockIdx.x; st < nsuper; st += gridDim.x) {
    const long long base = st * GM_PW;
    float a[GM_PT][KS];
    float m[GM_PT][4], l[GM_PT][4];
    int bidx[GM_PT][4];
#pragma unroll
    for (int t = 0; t < GM_PT; ++t)
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        m[t][i] = -INFINITY;
        l[t][i] = 0.f;
        bidx[t][i] = 0;
      }

    for (int ct = 0; ct < nct; ++ct) {
      const bool stage_a = nct > 1 || !astaged;
      __syncthreads();  // every reader of As / bS / Xs / lpS of the step before is done
      if (stage_a) {
        gm_stage<W, S, GM_CT>(As, p.A, (long long)ct * GM_CT, k, 2 * d, 0, d, p.vec, tid);
        gm_stage<W, S, GM_CT>(As + GM_CT * S, p.A, (long long)ct * GM_CT, k, 2 * d, d, d, p.vec, tid);
        if (tid < GM_CT) bS[tid] = ct * GM_CT + tid < k ? p.b[ct * GM_CT + tid] : -INFINITY;
        astaged = true;
      }
      if (ct == 0) gm_stage<W, S, GM_PW>(Xs, p.X, base, n, d, 0, d, p.vec, tid);
      __syncthreads();
      if (ct == 0) {
#pragma unroll
        for (int t = 0; t < GM_PT; ++t) {
          const float* xr = Xs + (wave * (16 * GM_PT) + t * 16 + col) * S + g;
#pragma unroll
          for (int ks = 0; ks < KS; ++ks) a[t][ks] = xr[4 * ks];
        }
      }
      const float* Ab = As + col * S + g;
      const int j0 = ct * GM_CT + col;
      const int nsub = min(4, (k - ct * GM_CT + 15) >> 4);
      if (nsub == 4) gm_online<KS, 4>(Ab, bS + col, j0, a, m, l, bidx);
      else if (nsub == 3) gm_online<KS, 3>(Ab, bS + col, j0, a, m, l, bidx);
      else if (nsub == 2) gm_online<KS, 2>(Ab, bS + col, j0, a, m, l, bidx);
      else gm_online<KS, 1>(Ab, bS + col, j0, a, m, l, bidx);
    }

    // the 16 lanes that share rows: merge (m, l), arg-max with the lowest index on ties
#pragma unroll
    for (int t = 0; t < GM_PT; ++t)
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        float mm = m[t][i], ls = l[t][i];
        int j = bidx[t][i];
#pragma unroll
        for (int x = 8; x >= 1; x >>= 1) {
          const float om = __shfl_xor(mm, x), ol = __shfl_xor(ls, x);
          const int oj = __shfl_xor(j, x);
          const float mx = fmaxf(mm, om);
          const float ms = mx == -INFINITY ? 0.f : mx;
          ls = ls * expf(mm - ms) + ol * expf(om - ms);
          if (om > mm || (om == mm && oj < j)) j = oj;
          mm = mx;
        }
        if (col == 0) {
          const int q = wave * (16 * GM_PT) + t * 16 + g * 4 + i;
          const float lp = mm + logf(ls);
          lpS[q] = lp;
          if (base + q < n) {
            p.logp[base + q] = lp;
            if (p.labels) p.labels[base + q] = min(max(j, 0), k - 1);
          }
        }
      }
    __syncthreads();
    if (tid < GM_PW && base + tid < n) myll += (double)lpS[tid];
  }

  if (p.ll) {
#pragma unroll
    for (int x = 32; x >= 1; x >>= 1) myll += __shfl_xor(myll, x);
    if (lane == 0 && myll != 0.0) unsafeAtomicAdd(p.ll, myll);
  }
}

// ---- pass 2: responsibilities in registers, R^T [X | X^2] on the matrix cores ----------------

struct GmStatArgs {
  const float* X;
  const float* A;
  const float* b;
  const float* logp;
  double* nk;
  double* s1;
  double* s2;
  long long n;
  int d, k;
  int vec;
  int slab;  // super-tiles per slab (<= GM_RUN / GM_PW)
};

__host__ __device__ constexpr int gm_stat_floats(int ks, int ns) {
  return 2 * 16 * ns * (4 * ks + 2) + GM_PW * (4 * ks + 4) + 16 * ns + GM_PW;
}

template <int KS, int NS>
__global__ __launch_bounds__(GM_THREADS) void gmm_stats_kernel(const GmStatArgs p) {
  constexpr int W = 4 * KS, SA = W + 2, SX = W + 4, NC = KS / 4, CT = 16 * NS, IW = 2 * W + 1;
  static_assert(CT * IW <= 2 * CT * SA + GM_PW * SX, "the flush image lies over the A and X tiles");
  extern __shared__ float gm_lds[];
  float* As = gm_lds;            // [2][CT][SA]
  float* Xs = As + 2 * CT * SA;  // [GM_PW][SX]
  float* bS = Xs + GM_PW * SX;   // [CT]
  float* lpS = bS + CT;          // [GM_PW]  logp, +inf past n
  float* img = gm_lds;           // [CT][IW]  at the flush: X columns, X^2 columns, nk

  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int col = lane & 15, g = lane >> 4;
  const int d = p.d, k = p.k;
  const long long n = p.n;
  const int ct = blockIdx.y;
  const long long nsuper = (n + GM_PW - 1) / GM_PW;
  const long long st0 = (long long)blockIdx.x * p.slab;
  const long long st1 = st0 + p.slab < nsuper ? st0 + p.slab : nsuper;

  gm_stage<W, SA, CT>(As, p.A, (long long)ct * CT, k, 2 * d, 0, d, p.vec, tid);
  gm_stage<W, SA, CT>(As + CT * SA, p.A, (long long)ct * CT, k, 2 * d, d, d, p.vec, tid);
  if (tid < CT) bS[tid] = ct * CT + tid < k ? p.b[ct * CT + tid] : -INFINITY;

  f32x4 acc1[NS][NC], acc2[NS][NC];
  float rs[NS];
#pragma unroll
  for (int s = 0; s < NS; ++s) {
    rs[s] = 0.f;
#pragma unroll
    for (int c = 0; c < NC; ++c) acc1[s][c] = acc2[s][c] = f32x4{0.f, 0.f, 0.f, 0.f};
  }

  for (long long st = st0; st < st1; ++st) {
    const long long base = st * GM_PW;
    __syncthreads();  // the readers of Xs / lpS of the super-tile before are done
    gm_stage<W, SX, GM_PW>(Xs, p.X, base, n, d, 0, d, p.vec, tid);
    if (tid < GM_PW) lpS[tid] = base + tid < n ? p.logp[base + tid] : INFINITY;
    __syncthreads();

    f32x4 r[NS][GM_PT];
    {
      float a[GM_PT][KS];
#pragma unroll
      for (int t = 0; t < GM_PT; ++t) {
        const float* xr = Xs + (wave * (16 * GM_PT) + t * 16 + col) * SX + g;
#pragma unroll
        for (int ks = 0; ks < KS; ++ks) a[t][ks] = xr[4 * ks];
      }
      gm_scores<KS, NS, SA, CT * SA>(As + col * SA + g, a, r);
    }
#pragma unroll
    for (int t = 0; t < GM_PT; ++t)
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const float lp = lpS[wave * (16 * GM_PT) + t * 16 + g * 4 + i];
#pragma unroll
        for (int s = 0; s < NS; ++s) {
          const float v = expf((r[s][t][i] + bS[s * 16 + col]) - lp);
          r[s][t][i] = v;
          rs[s] += v;
        }
      }
    // second product: k-step i of tile t contracts over the points 4 g' + i, g' = 0..3
#pragma unroll
    for (int t = 0; t < GM_PT; ++t)
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const float* xb = Xs + (wave * (16 * GM_PT) + t * 16 + g * 4 + i) * SX + col;
#pragma unroll
        for (int c = 0; c < NC; ++c) {
          const float x = xb[16 * c], x2 = x * x;
#pragma unroll
          for (int s = 0; s < NS; ++s) gm_mfma(r[s][t][i], x, acc1[s][c]);
#pragma unroll
          for (int s = 0; s < NS; ++s) gm_mfma(r[s][t][i], x2, acc2[s][c]);
        }
      }
  }

  // fold the four waves' blocks into one fp32 image, then widen and add
  __syncthreads();
  for (int w = 0; w < 4; ++w) {
    if (wave == w) {
#pragma unroll
      for (int s = 0; s < NS; ++s) {
#pragma unroll
        for (int c = 0; c < NC; ++c)
#pragma unroll
          for (int i = 0; i < 4; ++i) {
            float* q = img + (s * 16 + g * 4 + i) * IW + 16 * c + col;
            q[0] = (w ? q[0] : 0.f) + acc1[s][c][i];
            q[W] = (w ? q[W] : 0.f) + acc2[s][c][i];
          }
        float v = rs[s];
        v += __shfl_xor(v, 16);
        v += __shfl_xor(v, 32);
        if (g == 0) {
          float* q = img + (s * 16 + col) * IW + 2 * W;
          q[0] = (w ? q[0] : 0.f) + v;
        }
      }
    }
    __syncthreads();
  }
  for (int e = tid; e < CT * IW; e += GM_THREADS) {
    const int r = e / IW, cc = e % IW, j = ct * CT + r;
    const float v = img[e];
    if (j >= k || v == 0.f) continue;
    if (cc < W) {
      if (cc < d) unsafeAtomicAdd(&p.s1[(size_t)j * d + cc], (double)v);
    } else if (cc < 2 * W) {
      if (cc - W < d) unsafeAtomicAdd(&p.s2[(size_t)j * d + cc - W], (double)v);
    } else {
      unsafeAtomicAdd(&p.nk[j], (double)v);
    }
  }
}

// ---- host side -----------------------------------------------------------------------------

inline int gm_ksteps(int d) { return d <= 16 ? 4 : d <= 64 ? 16 : 32; }

struct GmDevice {
  int lds = 0, cus = 0;
};

inline const GmDevice* gm_device() {
  static GmDevice devs[64];
  int dev = 0;
  if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= 64) return nullptr;
  GmDevice& D = devs[dev];
  if (D.cus == 0) {
    int lds = 0, cus = 0;
    if (hipDeviceGetAttribute(&lds, hipDeviceAttributeMaxSharedMemoryPerBlock, dev) != hipSuccess ||
        hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess || cus <= 0)
      return nullptr;
    D.lds = lds < GM_LDS_MAX ? lds : GM_LDS_MAX;
    D.cus = cus;
  }
  return &D;
}

template <int KS>
int gm_launch_score(const GmScoreArgs& a, const GmDevice* D, hipStream_t s) {
  static bool lds_attr = false;  // dynamic LDS above 64 KiB must be allowed once
  const size_t lds = 4 * (size_t)gm_score_floats(KS);
  if (lds > (size_t)D->lds) return -3;
  if (!lds_attr) {
    (void)hipFuncSetAttribute((const void*)gmm_score_kernel<KS>, hipFuncAttributeMaxDynamicSharedMemorySize,
                              GM_LDS_MAX);
    lds_attr = true;
  }
  const long long nsuper = (a.n + GM_PW - 1) / GM_PW;
  long long wpc = GM_LDS_MAX / (long long)lds;
  wpc = wpc < 1 ? 1 : wpc > 2 ? 2 : wpc;
  const unsigned grid = (unsigned)(nsuper < wpc * D->cus ? nsuper : wpc * D->cus);
  hipLaunchKernelGGL((gmm_score_kernel<KS>), dim3(grid), dim3(GM_THREADS), lds, s, a);
  return (int)hipGetLastError();
}

template <int KS, int NS>
int gm_launch_stats(GmStatArgs a, const GmDevice* D, hipStream_t s) {
  static bool lds_attr = false;
  const size_t lds = 4 * (size_t)gm_stat_floats(KS, NS);
  if (lds > (size_t)D->lds) return -3;
  if (!lds_attr) {
    (void)hipFuncSetAttribute((const void*)gmm_stats_kernel<KS, NS>, hipFuncAttributeMaxDynamicSharedMemorySize,
                              GM_LDS_MAX);
    lds_attr = true;
  }
  const long long nsuper = (a.n + GM_PW - 1) / GM_PW;
  const int nct = (a.k + 16 * NS - 1) / (16 * NS);
  long long want = (4ll * D->cus + nct - 1) / nct;  // slabs that give every CU about four workgroups
  long long slab = (nsuper + want - 1) / want;
  slab = slab < 1 ? 1 : slab > GM_RUN / GM_PW ? GM_RUN / GM_PW : slab;
  const long long nslabs = (nsuper + slab - 1) / slab;
  if (nslabs > 0x7fffffffll) return -2;
  a.slab = (int)slab;
  hipLaunchKernelGGL((gmm_stats_kernel<KS, NS>), dim3((unsigned)nslabs, (unsigned)nct), dim3(GM_THREADS), lds, s, a);
  return (int)hipGetLastError();
}

template <int KS>
int gm_stats_ns(const GmStatArgs& a, const GmDevice* D, hipStream_t s) {
  // d > 64: a 64-component block of accumulators (256 registers) leaves no room
  // for the fragments, so the component tile is 32 there
  const int ns = (a.k + 15) / 16;
  if constexpr (KS <= 16) {
    if (ns >= 4) return gm_launch_stats<KS, 4>(a, D, s);
    if (ns == 3) return gm_launch_stats<KS, 3>(a, D, s);
  }
  if (ns >= 2) return gm_launch_stats<KS, 2>(a, D, s);
  return gm_launch_stats<KS, 1>(a, D, s);
}

inline bool gm_shape_ok(long long n, int d, int k) { return d >= 1 && d <= GM_MAXD && k >= 1 && k <= GM_MAXK && n >= 0; }

}  // namespace

extern "C" {

// Most points whose products one fp32 accumulator of the statistics pass sums.
int mr_gmm_run(void) { return GM_RUN; }

// A [k, 2d], b [k] from weights [k], means [k, d], variances [k, d] (all fp32).
int mr_gmm_prepare(const void* w, const void* M, const void* V, int d, int k, void* A, void* b, hipStream_t s) {
  if (!gm_shape_ok(0, d, k)) return -2;
  hipLaunchKernelGGL(gmm_prepare_kernel, dim3(k), dim3(64), 0, s, (const float*)w, (const float*)M, (const float*)V,
                     d, k, (float*)A, (float*)b);
  return (int)hipGetLastError();
}

// Pass 1: logp [n] fp32, optional labels [n] int32, optional ll += sum logp.
// -2: shape outside 1 <= d <= 128, 1 <= k <= 4096, n >= 0;  -3: LDS too small.
int mr_gmm_score(const void* X, const void* A, const void* b, long long n, int d, int k, void* logp, void* labels,
                 void* ll, hipStream_t s) {
  if (!gm_shape_ok(n, d, k)) return -2;
  if (n == 0) return 0;
  const GmDevice* D = gm_device();
  if (!D) return -1;
  GmScoreArgs a;
  a.X = (const float*)X;
  a.A = (const float*)A;
  a.b = (const float*)b;
  a.logp = (float*)logp;
  a.labels = (int*)labels;
  a.ll = (double*)ll;
  a.n = n;
  a.d = d;
  a.k = k;
  a.vec = (d % 4 == 0 && (((uintptr_t)X | (uintptr_t)A) & 15) == 0) ? 1 : 0;
  const int ks = gm_ksteps(d);
  if (ks == 32) return gm_launch_score<32>(a, D, s);
  if (ks == 16) return gm_launch_score<16>(a, D, s);
  return gm_launch_score<4>(a, D, s);
}

// Pass 2: nk [k], s1 [k, d], s2 [k, d] (float64) += the statistics under the
// logp pass 1 wrote for the same X, A, b.
int mr_gmm_stats(const void* X, const void* A, const void* b, const void* logp, long long n, int d, int k, void* nk,
                 void* s1, void* s2, hipStream_t s) {
  if (!gm_shape_ok(n, d, k)) return -2;
  if (n == 0) return 0;
  const GmDevice* D = gm_device();
  if (!D) return -1;
  GmStatArgs a;
  a.X = (const float*)X;
  a.A = (const float*)A;
  a.b = (const float*)b;
  a.logp = (const float*)logp;
  a.nk = (double*)nk;
  a.s1 = (double*)s1;
  a.s2 = (double*)s2;
  a.n = n;
  a.d = d;
  a.k = k;
  a.vec = (d % 4 == 0 && (((uintptr_t)X | (uintptr_t)A) & 15) == 0) ? 1 : 0;
  a.slab = 1;
  const int ks = gm_ksteps(d);
  if (ks == 32) return gm_stats_ns<32>(a, D, s);
  if (ks == 16) return gm_stats_ns<16>(a, D, s);
  return gm_stats_ns<4>(a, D, s);
}

}  // extern "C"
