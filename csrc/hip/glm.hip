// glm.hip — the Newton (IRLS) statistics of logistic regression in one pass over the points:
//
//   z_r = [x_r, 1]                       (X [n, d] fp32 row-major; p = d + 1 <= 128 columns, the last the intercept)
//   eta_r = z_r . beta                   mu_r = sigmoid(eta_r)       om_r = mu_r (1 - mu_r)
//   ll     += sum_r y_r eta_r - softplus(eta_r)                      (float64 [1])
//   g[c]   += sum_r (y_r - mu_r) z_rc                                (float64 [p])
//   H[i,j] += sum_r om_r z_ri z_rj                                   (float64 [p, p], both triangles)
//
// A weighted Gram matrix whose row weights depend on beta, so the sweep of gram.hip is reused for
// the operands and everything between the load and the product is new.
//
// Operands.  As in gram_rows_kernel, lane l = 16 g + m of a wave holds, for the four rows r0 .. r0 + 3
// of a step and every 16-column block b, f[b] = z[r0 + g][col(b, m)]: the A operand of block-row b
// and the B operand of block-column b of __builtin_amdgcn_mfma_f32_16x16x4f32 are that one register.
// IL = 1: col(b, m) = 16 b + m, 4-byte loads.  IL = 4: col(b, m) = 64 (b / 4) + 4 m + b % 4, one
// 16-byte load fills four blocks' registers; used when d % 4 == 0, X is 16-byte aligned and NB % 4
// == 0.  Column d is generated as 1.0f, columns >= p as 0, rows outside the run as 0: nothing but X
// and y is read.
//
// Per four-row step, new here:
// * eta.  beta's fragments bt[b] = beta[col(b, m)] stay in registers.  A lane forms f[0] bt[0], then
//   one fma per further block in ascending b; the 16 lanes of a row group finish with an xor
//   butterfly (1, 2, 4, 8).  Each step adds the same two numbers in both partners (fp32 addition
//   commutes), so all 16 lanes end with the same bits of eta_r.  A term passes at most NB + 4 roundings.
// * the link, gl_logistic: t = expf(-|eta|), mu = eta >= 0 ? 1 / (1 + t) : t / (1 + t) by IEEE
//   division, om = mu (1 - mu), softplus = max(eta, 0) + log1pf(t).  Saturates, never overflows;
//   eta = 0 gives mu = 0.5 and om = 0.25 exactly.
// * H: the A operand is fl32(om_r f[bi]) (one multiply per block and step), the B operand f[bj];
//   only the P = NB (NB + 1) / 2 blocks bi <= bj are multiplied.
// * g, off the matrix unit: gs[b] = fma(y_r - mu_r, f[b], gs[b]) per lane, NB fmas against P MFMAs.
// * ll: a per-lane fp32 sum of fma(y_r, eta_r, -softplus_r) over the lane's rows; the 16 lanes of a row
//   group hold the same sum and only the m = 0 lanes are counted, so a row counts once.
// * y[r]: a 4-byte load from a clamped in-bounds address, the same for the 16 lanes of a row group.
//
// Pipeline.  Two register buffers of UB steps: the next batch's loads are issued, then the next
// batch's (om, y - mu, ll) are formed, then the current batch's products: the exp / divide chain of batch
// k + 1 is independent of the MFMAs of batch k, so the scheduler is free to lay it between them.
//
// Widening and partials, as in gram.hip.  The four waves of a workgroup split the rows of the
// workgroup's slab.  Every RUN = 4096 rows they fold their accumulators into one fp32 image in LDS
// (a cell has then summed at most 1024 rows on the matrix unit and three more adds; a gradient or ll
// lane at most 256 rows, two shuffles and the three adds), and the image is added, widened, into the
// workgroup's float64 partial in the caller's workspace: P blocks of 256 in fragment order, then 16 NB
// gradient cells, then ll.  One owner thread per cell, plain loads and stores, no atomics.
// glm_reduce_kernel adds the partials IN SLAB ORDER into ll, g and H (which may hold a running state),
// un-permutes the interleave and writes every H value to both triangles; inside a diagonal block only
// the entries on or above the diagonal are used, so H is symmetric by construction.
//
// No host synchronisation, no allocation, no memset: capture-safe.  Compiler resource report (gfx950,
// -O3, packed fp32 ops off; no scratch in any kernel; LDS is static): profiles/glm/README.md.
#include <hip/hip_runtime.h>
#include <stdint.h>

typedef float f32x4 __attribute__((ext_vector_type(4)));

namespace {

constexpr int GL_THREADS = 256;  // 4 waves
constexpr int GL_MAXP = 128;
constexpr int GL_RUN = 4096;     // most rows one fp32 value sums before it is widened

struct GlArgs {
  const float* X;
  const float* y;
  const float* beta;
  double* ws;
  long long n;
  long long L;  // rows per slab
  int d, p;
};

__device__ __forceinline__ void gl_mfma(float a, float b, f32x4& c) {
  c = __builtin_amdgcn_mfma_f32_16x16x4f32(a, b, c, 0, 0, 0);
}

template <int IL>
__host__ __device__ __forceinline__ int gl_col(int b, int m) {
  return IL == 1 ? 16 * b + m : 64 * (b >> 2) + 4 * m + (b & 3);
}

__host__ __device__ constexpr int gl_cells(int nb) { return nb * (nb + 1) / 2 * 256 + 16 * nb + 1; }

// The logistic link of one row: the IRLS weight, the residual and the row's log-likelihood.  A later
// family replaces this function (and becomes a template parameter of the sweep).
struct GlRow {
  float om, res, ll;
};

__device__ __forceinline__ GlRow gl_logistic(float eta, float y) {
  const float t = expf(-fabsf(eta));  // in (0, 1]; 0 once |eta| is past ~104
  const float s = 1.f + t;
  const float mu = (eta >= 0.f ? 1.f : t) / s;
  return GlRow{mu * (1.f - mu), y - mu, fmaf(y, eta, -(fmaxf(eta, 0.f) + log1pf(t)))};
}

// f[u][b] = z[r + 4 u + g][col(b, m)] and yv[u] = y[r + 4 u + g]; rows >= lim give f = 0 (yv is then
// some in-bounds label, masked by the caller).  r is wave-uniform.  Addresses are (wave-uniform row
// pointer) + (32-bit lane offset), and every load is unconditional from a clamped in-bounds address.
template <int NB, int IL, int UB>
__device__ __forceinline__ void gl_load(const GlArgs& p, float (&f)[UB][NB], float (&yv)[UB], long long r,
                                        long long lim, int g, int m) {
#pragma unroll
  for (int u = 0; u < UB; ++u) {
    const long long base = r + 4 * u;
    const long long b0 = base < p.n ? base : p.n - 1;  // base >= n: the last row, masked below
    const long long left = p.n - 1 - b0;
    const int gg = g < left ? g : (int)left;
    const float* __restrict__ row = p.X + b0 * p.d;
    const bool ok = base + g < lim;
    yv[u] = p.y[b0 + gg];
    if constexpr (IL == 1) {
#pragma unroll
      for (int b = 0; b < NB; ++b) {
        const int c = 16 * b + m;
        const float x = row[(unsigned)(gg * p.d + (c < p.d ? c : 0))];
        f[u][b] = !ok ? 0.f : c < p.d ? x : c == p.d ? 1.f : 0.f;
      }
    } else {
#pragma unroll
      for (int q = 0; q < NB / 4; ++q) {
        const int c0 = 64 * q + 4 * m;  // d % 4 == 0: the quad lies in X or past it, and column d leads its quad
        const f32x4 v = *reinterpret_cast<const f32x4*>(row + (unsigned)(gg * p.d + (c0 < p.d ? c0 : 0)));
#pragma unroll
        for (int j = 0; j < 4; ++j)
          f[u][4 * q + j] = !ok ? 0.f : c0 < p.d ? v[j] : (c0 == p.d && j == 0) ? 1.f : 0.f;
      }
    }
  }
}

// The weights of a loaded batch: eta by fma chain and butterfly, then the link.  ll is summed here.
template <int NB, int UB>
__device__ __forceinline__ void gl_weights(const float (&f)[UB][NB], const float (&yv)[UB], const float (&bt)[NB],
                                           float (&om)[UB], float (&res)[UB], float& lls, long long r, long long lim,
                                           int g) {
#pragma unroll
  for (int u = 0; u < UB; ++u) {
    float eta = f[u][0] * bt[0];
#pragma unroll
    for (int b = 1; b < NB; ++b) eta = fmaf(f[u][b], bt[b], eta);
    eta += __shfl_xor(eta, 1);
    eta += __shfl_xor(eta, 2);
    eta += __shfl_xor(eta, 4);
    eta += __shfl_xor(eta, 8);
    const GlRow w = gl_logistic(eta, yv[u]);
    om[u] = w.om;  // a masked row has f = 0: its products vanish whatever om and res are
    res[u] = w.res;
    lls += r + 4 * u + g < lim ? w.ll : 0.f;
  }
}

template <int NB, int UB>
__device__ __forceinline__ void gl_products(const float (&f)[UB][NB], const float (&om)[UB], const float (&res)[UB],
                                            f32x4 (&acc)[NB * (NB + 1) / 2], float (&gs)[NB]) {
#pragma unroll
  for (int u = 0; u < UB; ++u) {
    int q = 0;
#pragma unroll
    for (int bi = 0; bi < NB; ++bi) {
      const float a = om[u] * f[u][bi];
#pragma unroll
      for (int bj = bi; bj < NB; ++bj) gl_mfma(a, f[u][bj], acc[q++]);
    }
#pragma unroll
    for (int b = 0; b < NB; ++b) gs[b] = fmaf(res[u], f[u][b], gs[b]);
  }
}

template <int NB, int IL>
__global__ __launch_bounds__(GL_THREADS) void glm_rows_kernel(const GlArgs p) {
  constexpr int P = NB * (NB + 1) / 2, NE = gl_cells(NB);
  constexpr int UB = NB >= 8 ? 2 : NB >= 4 ? 4 : 8;  // four-row steps per batch
  constexpr int BR = 4 * UB;                         // rows per batch
  constexpr int NBW = GL_RUN / (4 * BR);             // batches per wave and run
  static_assert(NBW % 2 == 0, "the batch loop is unrolled by two");
  __shared__ float img[NE];

  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);  // wave-uniform for the compiler too
  const int m = lane & 15, g = lane >> 4;
  const long long ra = (long long)blockIdx.x * p.L < p.n ? (long long)blockIdx.x * p.L : p.n;
  const long long rb = ra + p.L < p.n ? ra + p.L : p.n;
  double* __restrict__ part = p.ws + (size_t)blockIdx.x * NE;

  float bt[NB];
#pragma unroll
  for (int b = 0; b < NB; ++b) {
    const int c = gl_col<IL>(b, m);
    bt[b] = p.beta[c < p.p ? c : 0];
    if (c >= p.p) bt[b] = 0.f;
  }
  f32x4 acc[P];
  float gs[NB];

  const long long nrun = rb - ra > 0 ? (rb - ra + GL_RUN - 1) / GL_RUN : 1;
  for (long long run = 0; run < nrun; ++run) {
    const long long c0 = ra + run * GL_RUN;
    const long long lim = c0 + GL_RUN < rb ? c0 + GL_RUN : rb;
#pragma unroll
    for (int q = 0; q < P; ++q) acc[q] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int b = 0; b < NB; ++b) gs[b] = 0.f;
    float lls = 0.f;

    // this wave's batches start at c0 + (wave + 4 it) BR; the lane's rows are + 4 u + g.  A batch past
    // lim (the last prefetch) is masked everywhere: f = 0 and no ll.
    float fa[UB][NB], fb[UB][NB], ya[UB], yb[UB], oa[UB], ob[UB], sa[UB], sb[UB];
    long long r = c0 + (long long)wave * BR;
    gl_load<NB, IL, UB>(p, fa, ya, r, lim, g, m);
    gl_weights<NB, UB>(fa, ya, bt, oa, sa, lls, r, lim, g);
#pragma unroll 1
    for (int it = 0; it < NBW && c0 + (long long)(wave + 4 * it) * BR < lim; it += 2) {
      gl_load<NB, IL, UB>(p, fb, yb, r + 4 * BR, lim, g, m);
      gl_weights<NB, UB>(fb, yb, bt, ob, sb, lls, r + 4 * BR, lim, g);
      gl_products<NB, UB>(fa, oa, sa, acc, gs);
      gl_load<NB, IL, UB>(p, fa, ya, r + 8 * BR, lim, g, m);
      gl_weights<NB, UB>(fa, ya, bt, oa, sa, lls, r + 8 * BR, lim, g);
      gl_products<NB, UB>(fb, ob, sb, acc, gs);
      r += 8 * BR;
    }

    // fold the four waves into one fp32 image, then widen into the partial
    lls += __shfl_xor(lls, 16);
    lls += __shfl_xor(lls, 32);
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
          float s = gs[b];
          s += __shfl_xor(s, 16);
          s += __shfl_xor(s, 32);
          if (g == 0) {
            float* e = img + P * 256 + 16 * b + m;
            *e = (v ? *e : 0.f) + s;
          }
        }
        if (lane == 0) {
          float* e = img + NE - 1;
          *e = (v ? *e : 0.f) + lls;
        }
      }
      __syncthreads();
    }
    for (int e = tid; e < NE; e += GL_THREADS) part[e] = (run ? part[e] : 0.0) + (double)img[e];
  }
}

// ---- partials -> ll, g, H, in slab order ----------------------------------------------------

__global__ __launch_bounds__(GL_THREADS) void glm_reduce_kernel(const double* __restrict__ ws, int slabs, int nb,
                                                                int il, int p, double* __restrict__ ll,
                                                                double* __restrict__ gr, double* __restrict__ H) {
  const int P = nb * (nb + 1) / 2, NE = gl_cells(nb);
  const int e = blockIdx.x * GL_THREADS + threadIdx.x;
  if (e >= NE) return;
  double* out;
  double* mirror = nullptr;
  if (e < P * 256) {
    int blk = e >> 8, bi = 0;
    while (blk >= nb - bi) blk -= nb - bi++;  // row-major upper triangle: row bi holds nb - bi blocks
    const int bj = bi + blk, i = (e >> 6) & 3, lane = e & 63;
    const int a = 4 * (lane >> 4) + i, b = lane & 15;  // accumulator register i of lane: row 4 g + i, column m
    const int c1 = il == 1 ? gl_col<1>(bi, a) : gl_col<4>(bi, a);
    const int c2 = il == 1 ? gl_col<1>(bj, b) : gl_col<4>(bj, b);
    if (c1 >= p || c2 >= p || (bi == bj && a > b)) return;
    out = H + (size_t)c1 * p + c2;
    if (c1 != c2) mirror = H + (size_t)c2 * p + c1;
  } else if (e < NE - 1) {
    const int k = e - P * 256;
    const int c = il == 1 ? gl_col<1>(k >> 4, k & 15) : gl_col<4>(k >> 4, k & 15);
    if (c >= p) return;
    out = gr + c;
  } else {
    out = ll;
  }
  double sum = 0.0;
  for (int k = 0; k < slabs; ++k) sum += ws[(size_t)k * NE + e];
  *out += sum;
  if (mirror) *mirror += sum;
}

template <int NB, int IL>
void gl_launch(const GlArgs& a, unsigned slabs, hipStream_t s) {
  hipLaunchKernelGGL((glm_rows_kernel<NB, IL>), dim3(slabs), dim3(GL_THREADS), 0, s, a);
}

}  // namespace

extern "C" {

// Most rows one fp32 value sums before it is widened to float64.
int mr_glm_run(void) { return GL_RUN; }

// Bytes of the float64 partials of `slabs` workgroups at p = d + 1 columns (0: p or slabs out of range).
unsigned long long mr_glm_workspace_bytes(int p, int slabs) {
  if (p < 2 || p > GL_MAXP || slabs < 1) return 0;
  return 8ull * (unsigned long long)gl_cells((p + 15) / 16) * (unsigned long long)slabs;
}

// ll [1], g [d + 1], H [d + 1, d + 1] (float64) += the Newton statistics of logistic regression of y [n]
// on [X | 1] at beta [d + 1].  -2: shape outside 1 <= d <= 127, 0 <= n < 2^40, 1 <= slabs.
int mr_glm_newton(const void* X, const void* y, const void* beta, long long n, int d, int slabs, void* ws, void* ll,
                  void* g, void* H, hipStream_t stream) {
  if (d < 1 || d + 1 > GL_MAXP || n < 0 || n >= (1ll << 40) || slabs < 1) return -2;
  if (n == 0) return 0;
  GlArgs a;
  a.X = (const float*)X;
  a.y = (const float*)y;
  a.beta = (const float*)beta;
  a.ws = (double*)ws;
  a.n = n;
  a.L = (n + slabs - 1) / slabs;
  a.d = d;
  a.p = d + 1;
  const int nb = (a.p + 15) / 16;
  const int il = (d % 4 == 0 && ((uintptr_t)X & 15) == 0 && nb % 4 == 0) ? 4 : 1;
  const unsigned S = (unsigned)slabs;
  switch (il == 4 ? -nb : nb) {
    case 1: gl_launch<1, 1>(a, S, stream); break;
    case 2: gl_launch<2, 1>(a, S, stream); break;
    case 3: gl_launch<3, 1>(a, S, stream); break;
    case 4: gl_launch<4, 1>(a, S, stream); break;
    case 5: gl_launch<5, 1>(a, S, stream); break;
    case 6: gl_launch<6, 1>(a, S, stream); break;
    case 7: gl_launch<7, 1>(a, S, stream); break;
    case 8: gl_launch<8, 1>(a, S, stream); break;
    case -4: gl_launch<4, 4>(a, S, stream); break;
    case -8: gl_launch<8, 4>(a, S, stream); break;
    default: return -2;
  }
  int rc = (int)hipGetLastError();
  if (rc) return rc;
  const unsigned cells = (unsigned)gl_cells(nb);
  hipLaunchKernelGGL(glm_reduce_kernel, dim3((cells + GL_THREADS - 1) / GL_THREADS), dim3(GL_THREADS), 0, stream,
                     (const double*)ws, slabs, nb, il, a.p, (double*)ll, (double*)g, (double*)H);
  return (int)hipGetLastError();
}

}  // extern "C"
