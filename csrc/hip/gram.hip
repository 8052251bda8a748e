// gram.hip — second-moment statistics of a tall matrix on the fp32 matrix cores:
//
//   Z = [X | Y]  (X [n, d], optional Y [n, t], fp32 row-major; w = d + t <= 256)
//   zc[r, c] = fl32(Z[r, c] - shift[c])        (one fp32 subtraction; no shift: zc = Z)
//   s[c]    += sum_r zc[r, c]                  (float64 [w])
//   G[i, j] += sum_r zc[r, i] zc[r, j]         (float64 [w, w], both triangles)
//
// The contraction runs over the POINTS, not over the features, so the operand
// layout differs from every distance sweep of this library.
//
// Same-register operands.  __builtin_amdgcn_mfma_f32_16x16x4f32 wants lane l to
// hold A[M = l % 16][K = l / 16] and B[K = l / 16][N = l % 16].  For a 16 x 16
// block (bi, bj) of Z^T Z over the four rows r0 .. r0 + 3, A[M][K] = zc[r0 + K][col(bi, M)]
// and B[K][N] = zc[r0 + K][col(bj, N)]: lane l's A value of block-row b and its
// B value of block-column b are the SAME number, f[b] = zc[r0 + l / 16][col(b, l % 16)].
// One register per 16-column block is loaded and used on both sides; nothing
// is transposed, in LDS or anywhere else.
//
// Column interleave IL.  Which 16 columns make up block b is free (a column
// permutation permutes G).  IL = 1: col(b, m) = 16 b + m, 4-byte loads, a wave
// instruction reads 4 rows x 64 bytes.  IL = 4: col(b, m) = 64 (b / 4) + 4 m +
// b % 4, so a lane's 16-byte load of four adjacent columns yields the fragment
// registers of four blocks and a wave instruction reads 4 rows x 256 bytes.
// IL = 4 is used when d % 4 == 0, X is 16-byte aligned and the block count is a
// multiple of 4 (otherwise it would add all-zero blocks); Y columns are always
// 4-byte loads.  Columns >= w load as zero.
//
// Upper triangle only: with NB blocks of 16 columns, the P = NB (NB + 1) / 2
// blocks bi <= bj are multiplied; the reduction mirrors them.  Two kernels:
//
// * gram_rows_kernel (NB <= 8, w <= 128).  The four waves of a workgroup split
//   the ROWS of the workgroup's slab and each holds all P <= 36 accumulator
//   blocks.  Operands go from global memory straight to registers in batches
//   of UB four-row steps, the next batch in flight behind the products of the
//   current one (two register buffers).  No LDS on the hot path.  Every RUN =
//   4096 rows the four waves fold their blocks into one fp32 image in LDS (so
//   one fp32 value has summed at most 1024 rows on the matrix unit and three
//   more adds), and the workgroup adds the image, widened, into its float64
//   partial.  Column sums are per-lane fp32 sums of the fragment registers over
//   the same runs, folded over the four row groups with two shuffles.
//
// * gram_blocks_kernel (NB = 10, 12, 14, 16; w <= 256).  136 blocks do not fit
//   one wave, so the waves split the BLOCKS (block p of the row-major upper
//   triangle belongs to wave p % 4: 34 blocks at NB = 16) and share a tile of
//   32 rows staged once in LDS as zc.  Row stride = 16 (mod 64) floats, so the
//   four rows of a fragment read fall on disjoint banks.  With 16-byte loads
//   the X part of a tile is one contiguous chunk; the next tile's loads are
//   issued right after the barrier and stay in registers behind the 8 x 34
//   products of the current tile (the plan of kmeans_seed.hip).  Y columns,
//   padding, and X where 16-byte loads do not apply are filled in place
//   between the barriers.  Every 2048 rows each wave widens its own blocks
//   into the partial.
//
// Slabs.  The rows are cut into `slabs` contiguous slabs of ceil(n / slabs)
// rows, one workgroup each.  A workgroup owns one float64 partial (P blocks of
// 256 in fragment order, then 16 NB column sums) in the caller's workspace and
// updates it with plain loads and stores from a fixed owner thread per cell:
// no atomics.  gram_reduce_kernel then adds the partials IN SLAB ORDER into s
// and G (which may hold a running state) and writes each value to both
// triangles; inside a diagonal block only the entries on or above the diagonal
// are used, so G is symmetric by construction.  The result is a function of
// the inputs and `slabs` alone.
//
// No host synchronisation, no allocation, no memset: capture-safe.
//
// Compiler resource report (gfx950, -O3, packed fp32 ops off; no scratch in any
// kernel; LDS is static): see profiles/gram/README.md.
#include <hip/hip_runtime.h>
#include <stdint.h>

typedef float f32x4 __attribute__((ext_vector_type(4)));

namespace {

constexpr int GR_THREADS = 256;  // 4 waves
constexpr int GR_MAXW = 256;
constexpr int GR_RUN = 4096;     // most rows one fp32 value sums before it is widened
constexpr int GR_RUN_B = 2048;   // rows between two widenings of gram_blocks_kernel
constexpr int GR_TR = 32;        // rows of an LDS tile of gram_blocks_kernel
constexpr int GR_SMALL_NB = 8;   // most blocks gram_rows_kernel holds per wave

struct GrArgs {
  const float* X;
  const float* Y;
  const float* shift;
  double* ws;
  long long n;
  long long L;  // rows per slab
  int d, t, w;
  int vec;      // d % 4 == 0 and X 16-byte aligned
};

__device__ __forceinline__ void gr_mfma(float a, float b, f32x4& c) {
  c = __builtin_amdgcn_mfma_f32_16x16x4f32(a, b, c, 0, 0, 0);
}

template <int IL>
__host__ __device__ __forceinline__ int gr_col(int b, int m) {
  return IL == 1 ? 16 * b + m : 64 * (b >> 2) + 4 * m + (b & 3);
}

// Addresses are (wave-uniform row pointer) + (32-bit lane offset), so a load needs one address
// register, and every load is unconditional from a clamped in-bounds address: no divergent branch.
struct GrRows {
  const float* X;  // row b0 of X
  const float* Y;  // row b0 of Y (null when t = 0: never read)
  int rmax;        // n - 1 - b0: the largest row offset inside the matrix
};

// Rows from `base` on; base >= n is clamped to the last row (such rows are masked by the caller).
__device__ __forceinline__ GrRows gr_rows(const GrArgs& p, long long base) {
  const long long b0 = base < p.n ? base : p.n - 1;
  const long long left = p.n - 1 - b0;
  return GrRows{p.X + b0 * p.d, p.Y + b0 * p.t, (int)(left < 1024 ? left : 1024)};
}

// Z[b0 + r, c] (not shifted); zero for c >= w.
__device__ __forceinline__ float gr_elem(const GrArgs& p, const GrRows& R, int r, int c) {
  const bool inx = c < p.d, iny = !inx && c < p.w;
  float z = R.X[(unsigned)(r * p.d + (inx ? c : 0))];
  z = inx ? z : 0.f;
  if (p.t > 0) {
    const float y = R.Y[(unsigned)(r * p.t + (iny ? c - p.d : 0))];
    z = iny ? y : z;
  }
  return z;
}

// Z[b0 + r, c0 .. c0 + 3] with one 16-byte load where the quad lies in X (d % 4 == 0, X aligned).
__device__ __forceinline__ f32x4 gr_quad(const GrArgs& p, const GrRows& R, int r, int c0) {
  const bool inx = c0 < p.d;
  f32x4 v = *reinterpret_cast<const f32x4*>(R.X + (unsigned)(r * p.d + (inx ? c0 : 0)));
  if (!inx) v = f32x4{0.f, 0.f, 0.f, 0.f};
  if (p.t > 0) {
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const int c = c0 + j;
      const bool iny = !inx && c < p.w;
      const float y = R.Y[(unsigned)(r * p.t + (iny ? c - p.d : 0))];
      v[j] = iny ? y : v[j];
    }
  }
  return v;
}

// ---- w <= 128: waves split the rows --------------------------------------------------------

// f[u][b] = zc[r + 4 u + g][col(b, m)], zero for rows >= lim.  r is wave-uniform.
template <int NB, int IL, int UB>
__device__ __forceinline__ void gr_load(const GrArgs& p, float (&f)[UB][NB], const float (&sh)[NB], long long r,
                                        long long lim, int g, int m) {
#pragma unroll
  for (int u = 0; u < UB; ++u) {
    const GrRows R = gr_rows(p, r + 4 * u);
    const bool ok = r + 4 * u + g < lim;
    const int gg = g < R.rmax ? g : R.rmax;
    if constexpr (IL == 1) {
#pragma unroll
      for (int b = 0; b < NB; ++b) {
        const float z = gr_elem(p, R, gg, 16 * b + m);
        f[u][b] = ok ? z - sh[b] : 0.f;
      }
    } else {
#pragma unroll
      for (int q = 0; q < NB / 4; ++q) {
        const f32x4 v = gr_quad(p, R, gg, 64 * q + 4 * m);
#pragma unroll
        for (int j = 0; j < 4; ++j) f[u][4 * q + j] = ok ? v[j] - sh[4 * q + j] : 0.f;
      }
    }
  }
}

template <int NB, int UB>
__device__ __forceinline__ void gr_products(const float (&f)[UB][NB], f32x4 (&acc)[NB * (NB + 1) / 2],
                                            float (&cs)[NB]) {
#pragma unroll
  for (int u = 0; u < UB; ++u) {
    int q = 0;
#pragma unroll
    for (int bi = 0; bi < NB; ++bi)
#pragma unroll
      for (int bj = bi; bj < NB; ++bj) gr_mfma(f[u][bi], f[u][bj], acc[q++]);
#pragma unroll
    for (int b = 0; b < NB; ++b) cs[b] += f[u][b];
  }
}

template <int NB, int IL>
__global__ __launch_bounds__(GR_THREADS) void gram_rows_kernel(const GrArgs p) {
  constexpr int P = NB * (NB + 1) / 2, NE = P * 256 + 16 * NB;
  constexpr int UB = NB >= 8 ? 2 : NB >= 4 ? 4 : NB >= 2 ? 8 : 16;  // four-row steps per batch
  constexpr int BR = 4 * UB;                                         // rows per batch
  constexpr int NBW = GR_RUN / (4 * BR);                             // batches per wave and run
  static_assert(NBW % 2 == 0, "the batch loop is unrolled by two");
  __shared__ float img[NE];

  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);  // wave-uniform for the compiler too
  const int m = lane & 15, g = lane >> 4;
  const long long ra = (long long)blockIdx.x * p.L < p.n ? (long long)blockIdx.x * p.L : p.n;
  const long long rb = ra + p.L < p.n ? ra + p.L : p.n;
  double* __restrict__ part = p.ws + (size_t)blockIdx.x * NE;

  float sh[NB];
#pragma unroll
  for (int b = 0; b < NB; ++b) {
    const int c = gr_col<IL>(b, m);
    sh[b] = (p.shift && c < p.w) ? p.shift[c] : 0.f;
  }
  f32x4 acc[P];
  float cs[NB];

  const long long nrun = rb - ra > 0 ? (rb - ra + GR_RUN - 1) / GR_RUN : 1;
  for (long long run = 0; run < nrun; ++run) {
    const long long c0 = ra + run * GR_RUN;
    const long long lim = c0 + GR_RUN < rb ? c0 + GR_RUN : rb;
#pragma unroll
    for (int q = 0; q < P; ++q) acc[q] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int b = 0; b < NB; ++b) cs[b] = 0.f;

    // this wave's batches start at c0 + (wave + 4 it) BR; the lane's rows are + 4 u + g
    float fa[UB][NB], fb[UB][NB];
    long long r = c0 + (long long)wave * BR;
    gr_load<NB, IL, UB>(p, fa, sh, r, lim, g, m);
#pragma unroll 1
    for (int it = 0; it < NBW && c0 + (long long)(wave + 4 * it) * BR < lim; it += 2) {
      gr_load<NB, IL, UB>(p, fb, sh, r + 4 * BR, lim, g, m);
      gr_products<NB, UB>(fa, acc, cs);
      gr_load<NB, IL, UB>(p, fa, sh, r + 8 * BR, lim, g, m);
      gr_products<NB, UB>(fb, acc, cs);
      r += 8 * BR;
    }

    // fold the four waves into one fp32 image, then widen into the partial
    __syncthreads();
    for (int v = 0; v < 4; ++v) {
      if (wave == v) {
#pragma unroll
        for (int q = 0; q < P; ++q) {
#pragma unroll
          for (int i = 0; i < 4; ++i) {
            float* e = img + (q * 4 + i) * 64 + lane;
            *e = (v ? *e : 0.f) + acc[q][i];
          }
          // four blocks at a time: left alone, the scheduler hoists all 4 P reads (4 P registers)
          if (q % 4 == 3) __builtin_amdgcn_sched_barrier(0);
        }
#pragma unroll
        for (int b = 0; b < NB; ++b) {
          float s = cs[b];
          s += __shfl_xor(s, 16);
          s += __shfl_xor(s, 32);
          if (g == 0) {
            float* e = img + P * 256 + 16 * b + m;
            *e = (v ? *e : 0.f) + s;
          }
        }
      }
      __syncthreads();
    }
    for (int e = tid; e < NE; e += GR_THREADS) part[e] = (run ? part[e] : 0.0) + (double)img[e];
  }
}

// ---- w > 128: waves split the blocks, one LDS tile of rows ---------------------------------

__host__ __device__ constexpr int gr_stride(int wp) { return wp + ((16 - wp % 64) + 64) % 64; }

// f[b] = tile row [col(b, m)]
template <int NB, int IL>
__device__ __forceinline__ void gr_fragments(const float* __restrict__ tr, int m, float (&f)[NB]) {
  if constexpr (IL == 1) {
#pragma unroll
    for (int b = 0; b < NB; ++b) f[b] = tr[16 * b + m];
  } else {
#pragma unroll
    for (int q = 0; q < NB / 4; ++q) {
      const f32x4 v = *reinterpret_cast<const f32x4*>(tr + 64 * q + 4 * m);
#pragma unroll
      for (int j = 0; j < 4; ++j) f[4 * q + j] = v[j];
    }
  }
}

template <int NB, int IL, int V>
__device__ __forceinline__ void gr_tile_products(const float* __restrict__ tile, int g, int m,
                                                 f32x4 (&acc)[(NB * (NB + 1) / 2 + 3) / 4], float (&cs)[(NB + 3) / 4]) {
  constexpr int S = gr_stride(16 * NB);
  // the fragments of step k + 1 are read from LDS behind the products of step k
  float f[NB], fn[NB];
  gr_fragments<NB, IL>(tile + g * S, m, f);
#pragma unroll 1
  for (int k = 0; k < GR_TR / 4; ++k) {
    gr_fragments<NB, IL>(tile + (4 * (k + 1 < GR_TR / 4 ? k + 1 : k) + g) * S, m, fn);
    int q = 0;
#pragma unroll
    for (int bi = 0; bi < NB; ++bi)
#pragma unroll
      for (int bj = bi; bj < NB; ++bj) {
        if (q % 4 == V) gr_mfma(f[bi], f[bj], acc[q / 4]);
        ++q;
      }
#pragma unroll
    for (int b = 0; b < NB; ++b) {
      if (b % 4 == V) cs[b / 4] += f[b];
      f[b] = fn[b];
    }
  }
}

template <int NB, int IL>
__global__ __launch_bounds__(GR_THREADS) void gram_blocks_kernel(const GrArgs p) {
  constexpr int WP = 16 * NB, S = gr_stride(WP), NQ = GR_TR * (WP / 4) / GR_THREADS;
  constexpr int P = NB * (NB + 1) / 2, PW = (P + 3) / 4, SB = (NB + 3) / 4, NE = P * 256 + 16 * NB;
  static_assert(NQ * GR_THREADS * 4 == GR_TR * WP && S % 4 == 0, "whole 16-byte quads per thread");
  __shared__ __attribute__((aligned(16))) float tile[GR_TR * S];
  __shared__ __attribute__((aligned(16))) float shS[WP];

  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);  // wave-uniform for the compiler too
  const int m = lane & 15, g = lane >> 4;
  const long long ra = (long long)blockIdx.x * p.L < p.n ? (long long)blockIdx.x * p.L : p.n;
  const long long rb = ra + p.L < p.n ? ra + p.L : p.n;
  double* __restrict__ part = p.ws + (size_t)blockIdx.x * NE;

  for (int c = tid; c < WP; c += GR_THREADS) shS[c] = (p.shift && c < p.w) ? p.shift[c] : 0.f;

  f32x4 acc[PW];
  float cs[SB];
#pragma unroll
  for (int q = 0; q < PW; ++q) acc[q] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
  for (int b = 0; b < SB; ++b) cs[b] = 0.f;

  // Staging.  With 16-byte loads the X part of a tile is one contiguous chunk of GR_TR d floats; quad
  // k of this thread is floats 4 e .. 4 e + 3 of it (e = tid + 256 k), prefetched into registers one
  // tile ahead and stored at tile[row][column] = loff[k].  Everything else (Y columns, padding,
  // and all of X where 16-byte loads do not apply) is filled in place between the barriers.
  int loff[NQ];
  f32x4 pre[NQ];
#pragma unroll
  for (int k = 0; k < NQ; ++k) {
    const int i = 4 * (tid + GR_THREADS * k);
    loff[k] = (p.vec && i < GR_TR * p.d) ? (i / p.d) * S + i % p.d : -1;
  }
  auto live_floats = [&](long long base) {  // floats of the chunk that lie inside the slab
    const long long left = rb - base;
    return (int)(left < 0 ? 0 : left < GR_TR ? left : GR_TR) * p.d;
  };
  auto fetch = [&](long long base) {
    if (!p.vec) return;
    const float* src = p.X + (base < p.n ? base : p.n - 1) * p.d;  // wave-uniform; >= 4 floats are readable
    const int live = live_floats(base);
#pragma unroll
    for (int k = 0; k < NQ; ++k) {
      const int i = 4 * (tid + GR_THREADS * k);
      pre[k] = *reinterpret_cast<const f32x4*>(src + (unsigned)(i < live ? i : 0));
    }
  };
  const int cf = p.vec ? p.d : 0, nc = WP - cf;  // columns cf .. WP - 1 are filled in place

  const long long ntile = rb - ra > 0 ? (rb - ra + GR_TR - 1) / GR_TR : 1;
  constexpr int TPR = GR_RUN_B / GR_TR;  // tiles per run
  fetch(ra);
  for (long long tl = 0; tl < ntile; ++tl) {
    const long long base = ra + tl * GR_TR;
    __syncthreads();  // the readers of the tile before are done (and shS is written)
    const int live = live_floats(base);
#pragma unroll
    for (int k = 0; k < NQ; ++k) {
      if (loff[k] < 0) continue;
      const int i = 4 * (tid + GR_THREADS * k);
      const f32x4 s4 = *reinterpret_cast<const f32x4*>(shS + loff[k] % S);
      f32x4 v;
#pragma unroll
      for (int j = 0; j < 4; ++j) v[j] = i < live ? pre[k][j] - s4[j] : 0.f;
      *reinterpret_cast<f32x4*>(tile + loff[k]) = v;
    }
    for (int e = tid; e < GR_TR * nc; e += GR_THREADS) {
      const int r = e / nc, c = cf + e % nc;
      const long long row = base + r;
      float v = 0.f;
      if (row < rb && c < p.w) v = (c < p.d ? p.X[row * p.d + c] : p.Y[row * p.t + (c - p.d)]) - shS[c];
      tile[r * S + c] = v;
    }
    __syncthreads();
    fetch(base + GR_TR);  // in flight behind the products; rows >= rb are masked at the store
    if (wave == 0) gr_tile_products<NB, IL, 0>(tile, g, m, acc, cs);
    else if (wave == 1) gr_tile_products<NB, IL, 1>(tile, g, m, acc, cs);
    else if (wave == 2) gr_tile_products<NB, IL, 2>(tile, g, m, acc, cs);
    else gr_tile_products<NB, IL, 3>(tile, g, m, acc, cs);

    if ((tl + 1) % TPR == 0 || tl + 1 == ntile) {  // widen this wave's own blocks
      const bool first = tl < TPR;
      // block 4 q + wave, register i, this lane.  The base is made opaque here so that the 4 PW
      // addresses are formed at the flush, not hoisted out of the tile loop into 8 PW registers.
      double* pw = part + wave * 256 + lane;
      asm volatile("" : "+v"(pw));
#pragma unroll
      for (int q = 0; q < PW; ++q) {
        const int blk = 4 * q + wave;
        if (blk < P) {
#pragma unroll
          for (int i = 0; i < 4; ++i) {
            double* e = pw + (q * 16 + i) * 64;
            *e = (first ? 0.0 : *e) + (double)acc[q][i];
          }
        }
        acc[q] = f32x4{0.f, 0.f, 0.f, 0.f};
        // four blocks at a time: left alone, the scheduler hoists every load (8 registers a block)
        if (q % 4 == 3) __builtin_amdgcn_sched_barrier(0);
      }
#pragma unroll
      for (int b = 0; b < SB; ++b) {
        float s = cs[b];
        s += __shfl_xor(s, 16);
        s += __shfl_xor(s, 32);
        const int blk = 4 * b + wave;
        if (blk < NB && g == 0) {
          double* e = part + P * 256 + 16 * blk + m;
          *e = (first ? 0.0 : *e) + (double)s;
        }
        cs[b] = 0.f;
      }
    }
  }
}

// ---- partials -> s, G, in slab order --------------------------------------------------------

__global__ __launch_bounds__(GR_THREADS) void gram_reduce_kernel(const double* __restrict__ ws, int slabs, int nb,
                                                                 int il, int w, double* __restrict__ s,
                                                                 double* __restrict__ G) {
  const int P = nb * (nb + 1) / 2, NE = P * 256 + 16 * nb;
  const int e = blockIdx.x * GR_THREADS + threadIdx.x;
  if (e >= NE) return;
  double* out;
  double* mirror = nullptr;
  if (e < P * 256) {
    int blk = e >> 8, bi = 0;
    while (blk >= nb - bi) blk -= nb - bi++;  // row-major upper triangle: row bi holds nb - bi blocks
    const int bj = bi + blk, i = (e >> 6) & 3, lane = e & 63;
    const int a = 4 * (lane >> 4) + i, b = lane & 15;  // accumulator register i of lane: row 4 g + i, column m
    const int c1 = il == 1 ? gr_col<1>(bi, a) : gr_col<4>(bi, a);
    const int c2 = il == 1 ? gr_col<1>(bj, b) : gr_col<4>(bj, b);
    if (c1 >= w || c2 >= w || (bi == bj && a > b)) return;
    out = G + (size_t)c1 * w + c2;
    if (c1 != c2) mirror = G + (size_t)c2 * w + c1;
  } else {
    const int k = e - P * 256;
    const int c = il == 1 ? gr_col<1>(k >> 4, k & 15) : gr_col<4>(k >> 4, k & 15);
    if (c >= w) return;
    out = s + c;
  }
  double sum = 0.0;
  for (int k = 0; k < slabs; ++k) sum += ws[(size_t)k * NE + e];
  *out += sum;
  if (mirror) *mirror += sum;
}

// ---- host side -----------------------------------------------------------------------------

// Blocks of 16 columns the kernel for width w works on: ceil(w / 16) up to 8, then rounded up to even.
inline int gr_blocks(int w) {
  const int nb = (w + 15) / 16;
  return nb <= GR_SMALL_NB ? nb : (nb + 1) & ~1;
}

inline size_t gr_partial_doubles(int w) {
  const int nb = gr_blocks(w);
  return (size_t)(nb * (nb + 1) / 2) * 256 + 16 * (size_t)nb;
}

template <int NB, int IL>
void gr_launch(const GrArgs& a, unsigned slabs, hipStream_t s) {
  if constexpr (NB <= GR_SMALL_NB)
    hipLaunchKernelGGL((gram_rows_kernel<NB, IL>), dim3(slabs), dim3(GR_THREADS), 0, s, a);
  else
    hipLaunchKernelGGL((gram_blocks_kernel<NB, IL>), dim3(slabs), dim3(GR_THREADS), 0, s, a);
}

}  // namespace

extern "C" {

// Most rows one fp32 value sums before it is widened to float64.
int mr_gram_run(void) { return GR_RUN; }

// Bytes of the float64 partials of `slabs` workgroups at width w (0: w or slabs out of range).
unsigned long long mr_gram_workspace_bytes(int w, int slabs) {
  if (w < 1 || w > GR_MAXW || slabs < 1) return 0;
  return 8ull * gr_partial_doubles(w) * (unsigned long long)slabs;
}

// s [w], G [w, w] (float64) += the moments of zc = [X | Y] - shift.  Y (t > 0) and shift may be null.
// -2: shape outside 1 <= d, 0 <= t, d + t <= 256, 0 <= n < 2^40, 1 <= slabs < 2^31.
int mr_gram_moments(const void* X, const void* Y, const void* shift, long long n, int d, int t, int slabs, void* ws,
                    void* s, void* G, hipStream_t stream) {
  if (d < 1 || t < 0 || d + t > GR_MAXW || n < 0 || n >= (1ll << 40) || slabs < 1) return -2;
  if (t > 0 && !Y) return -2;
  if (n == 0) return 0;
  GrArgs a;
  a.X = (const float*)X;
  a.Y = (const float*)Y;
  a.shift = (const float*)shift;
  a.ws = (double*)ws;
  a.n = n;
  a.L = (n + slabs - 1) / slabs;
  a.d = d;
  a.t = t;
  a.w = d + t;
  a.vec = (d % 4 == 0 && ((uintptr_t)X & 15) == 0) ? 1 : 0;
  const int nb = gr_blocks(a.w);
  const int il = (a.vec && nb % 4 == 0) ? 4 : 1;
  const unsigned S = (unsigned)slabs;
  switch (il == 4 ? -nb : nb) {
    case 1: gr_launch<1, 1>(a, S, stream); break;
    case 2: gr_launch<2, 1>(a, S, stream); break;
    case 3: gr_launch<3, 1>(a, S, stream); break;
    case 4: gr_launch<4, 1>(a, S, stream); break;
    case 5: gr_launch<5, 1>(a, S, stream); break;
    case 6: gr_launch<6, 1>(a, S, stream); break;
    case 7: gr_launch<7, 1>(a, S, stream); break;
    case 8: gr_launch<8, 1>(a, S, stream); break;
    case 10: gr_launch<10, 1>(a, S, stream); break;
    case 12: gr_launch<12, 1>(a, S, stream); break;
    case 14: gr_launch<14, 1>(a, S, stream); break;
    case 16: gr_launch<16, 1>(a, S, stream); break;
    case -4: gr_launch<4, 4>(a, S, stream); break;
    case -8: gr_launch<8, 4>(a, S, stream); break;
    case -12: gr_launch<12, 4>(a, S, stream); break;
    case -16: gr_launch<16, 4>(a, S, stream); break;
    default: return -2;
  }
  int rc = (int)hipGetLastError();
  if (rc) return rc;
  const unsigned cells = (unsigned)gr_partial_doubles(a.w);
  hipLaunchKernelGGL(gram_reduce_kernel, dim3((cells + GR_THREADS - 1) / GR_THREADS), dim3(GR_THREADS), 0, stream,
                     (const double*)ws, slabs, nb, il, a.w, (double*)s, (double*)G);
  return (int)hipGetLastError();
}

}  // extern "C"
