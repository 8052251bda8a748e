// knn.hip — brute-force k-nearest neighbours under the squared Euclidean
// metric: a fused fp32-MFMA distance sweep that keeps the K best (distance,
// index) pairs of every query in LDS, and a merge kernel for partial lists.
// Self-contained, like kmeans.hip, kmeans_seed.hip and gmm.hip; the n x q
// distance matrix never exists.
//
// mr_knn_search.  Q [nq, d] fp32, X [n, d] fp32, 1 <= d <= 512, 1 <= K <= 64,
// nq >= 0, 0 <= n < 2^31, running state dist fp32 [nq, K] / idx int64 [nq, K]:
//
//   score(i, j) = fl(|x_j|^2) - 2 q_i . x_j       (one fma on the MFMA chain)
//   dist(i, j)  = max(0, fl(fl(|q_i|^2) + score(i, j)))
//   the state becomes the K smallest (dist, idx) pairs, lexicographic, of the
//   state and {(dist(i, j), base + j)}; free slots hold (+inf, -1).
//
// dist(i, j) depends on row i of Q and row j of X alone: the MFMA chain of a
// pair runs over its d products in column order whatever the tile, the slab or
// the d-chunk (the chunks of d > 128 add into the same accumulator, zero
// padding adds exact zeros), and |q|^2, |x|^2 are formed per row.  The list
// code then only orders integers, so the result is the same bits for every
// slab count and every way of cutting X into calls.
//
// Keys.  A (dist, local index) pair is one u64: dist >= 0, so its bit pattern
// (sign cleared: max(0, -0)) is already its order-preserving integer image and
// is the high word; the row index j is the low word.  0xFFFFFFFF FFFFFFFF is
// the free slot.  Smaller key = lexicographically smaller (dist, index).
//
// Sweep kernel.  Grid (ceil(nq / 128), S).  A workgroup of 4 waves owns 128
// queries, wave w the two 16-row MFMA tiles at rows [32 w, 32 w + 32), and the
// slab of 64-row X tiles that blockIdx.y selects (tiles split evenly over the
// slabs, the remainder to the first ones).
//
//   * Q is staged in LDS coalesced along d (rows padded to a stride of 4 KS + 2
//     floats, = 2 (mod 64) for KS = 16 and 32: the 16 rows x 4 k-groups a wave
//     reads with one ds_read fall on banks 2 row + g (+ 4 ks), 64 lanes on 34
//     banks, at most 2-way), |q|^2 is one fma chain per row in column order,
//     and each lane lifts a[t][ks] = Q[row = lane & 15][4 ks + (lane >> 4)]
//     into registers for the whole sweep (d <= 128).  d > 128 runs in d-chunks
//     of 64 (KS = 16): the Q chunk is re-staged beside every X chunk.
//   * X tiles: a thread holds its share of the NEXT tile in registers (16-byte
//     loads issued before the MFMA sweep of the current tile, written to LDS
//     after it).  |x|^2 of a staged row is taken by 4 threads, thread r of them
//     one fma chain over the columns c = r (mod 4) in column order, combined
//     (s0 + s1) + (s2 + s3); the chunks of d > 128 add in chunk order.  (One
//     64-lane chain per tile would leave three waves idle for 4 KS dependent
//     fmas; the bound gamma_{d+2} |x|^2 holds for either order.)
//   * v_mfma_f32_16x16x4_f32: acc[s][t] (4 column tiles x 2 row tiles) holds
//     q . x; lane (col, g) owns queries 4 g + i, i < 4, of row tile t and point
//     16 s + col of the X tile.
//   * Selection is wave-private: the lists, thresholds, pending buffers and
//     counters of a wave's 32 queries are touched by that wave only, so a
//     compaction needs no workgroup barrier.  A lane keeps, for its 8 rows,
//     |q|^2 and the threshold tau (the distance of the K-th key; NaN while the
//     list has free slots) in registers.  Points reach a slab's sweep in
//     ascending index order, so a point whose distance EQUALS tau loses to the
//     K-th key on the index: the test is !(fl(|q|^2 + score) >= tau), 3 VALU
//     operations a pair.  A pair that passes is clamped, made a key, checked
//     against the row limit and appended to its query's pending buffer through
//     an LDS counter (ds_add_rtn).
//   * Compaction.  P = 32 pending keys a query; a column tile adds at most 16
//     to a query, so after every column tile in which a lane of the wave
//     appended, the wave looks at its 32 counters and compacts every query that
//     holds more than TRIG = 16: no buffer can overflow on the next column
//     tile.  The wave merges one query at a time: lane i holds list key L_i
//     (sorted), lane j < c pending key p_j; the loop over j broadcasts p_j
//     (readlane), ballots L_i < p_j and p_j' < p_j, and gives rank(p_j) =
//     popcount + popcount, rank(L_i) = i + c - #{j : L_i < p_j} (keys are
//     distinct).  Keys with rank < K are stored at their rank; the lane that
//     holds rank K - 1 refreshes tau.  Everything is read into registers before
//     the first store, so the merge is in place.  At the end of the slab every
//     query with pending keys is compacted and the lists go to
//     workspace[slab][query][K] as u64 keys.
//   * LDS (bytes; S = 4 KS + 2): X tile 256 S, |x|^2 256, |q|^2 512, tau 512,
//     counters 512, then the Q tile (512 S) and, for d <= 128 in the SAME bytes
//     (Q is dead once the fragments are lifted), the list plane 1024 K and the
//     pending plane 128 x 33 x 8 = 33 792.  Pending rows are padded to 33 keys:
//     the 4 queries one append instruction touches (rows 4 g + i) are 4 rows
//     apart = 8 banks, so equal counters do not collide.  List rows are dense:
//     a wave reads one list with consecutive lanes.
//       KS = 32, K = 64:          33 280 + 1 792 + max(66 560, 65 536 + 33 792) = 134 400
//       KS = 16 chunks, K = 64:   16 896 + 1 792 + 33 792 + 65 536 + 33 792     = 151 808
//       KS = 4,  K = 1:            4 608 + 1 792 + max(9 216, 1 024 + 33 792)   =  41 216
//     all within the 160 KiB of a CU.
//
// Merge kernel.  One wave a query: lane i holds entry i of the running list
// (dist image, int64 index).  Every further sorted list (the second state of
// mr_knn_merge, then the S slab lists with idx = base + low word) is merged by
// ranks: rank(a_i) = i + #{b < a_i}, rank(b_i) = i + #{a <= b_i}, both counted
// in one loop of readlane broadcasts; entries with rank < K move to their rank
// through a per-wave LDS row.  Input slots with idx < 0 are free slots.
//
// Compiler resource report (gfx950, -O3, -Rpass-analysis=kernel-resource-usage):
// see profiles/knn/README.md; no kernel uses scratch.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef float f32x2 __attribute__((ext_vector_type(2)));

namespace {

constexpr int KN_THREADS = 256;  // 4 waves
constexpr int KN_QB = 128;       // queries per workgroup
constexpr int KN_XT = 64;        // X rows per LDS tile (4 MFMA column tiles)
constexpr int KN_MAXD = 512, KN_MAXK = 64;
constexpr int KN_P = 32;         // pending keys per query
constexpr int KN_PS = KN_P + 1;  // padded pending row (keys)
constexpr int KN_TRIG = KN_P - 16;
constexpr int KN_MAXS = 65535;
constexpr int KN_LDS_MAX = 160 * 1024;
constexpr uint32_t KN_FREE = 0xFFFFFFFFu;
constexpr unsigned long long KN_FREE64 = ~0ull;

struct KnArgs {
  const float* Q;
  const float* X;
  unsigned long long* ws;  // [S][nq][K] keys
  long long nq;
  int n, d, k, slabs;
  int vecq, vecx;  // d % 4 == 0 and the base 16-byte aligned
};

__host__ __device__ constexpr int kn_stride(int ks) { return 4 * ks + 2; }
__host__ __device__ constexpr size_t kn_lds_bytes(int ks, bool multi, int k) {
  const size_t qt = 4u * KN_QB * kn_stride(ks), sel = 8u * KN_QB * (size_t)k + 8u * KN_QB * KN_PS;
  return 4u * KN_XT * kn_stride(ks) + 4u * (KN_XT + 3 * KN_QB) + (multi ? qt + sel : (qt > sel ? qt : sel));
}

// LDS operations of one wave execute in order; this keeps the compiler from
// moving or caching them across a hand-over between lanes of the wave.
__device__ __forceinline__ void kn_wave_sync() {
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

__device__ __forceinline__ unsigned long long kn_bcast64(unsigned long long v, int j) {
  const uint32_t lo = (uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)v, j);
  const uint32_t hi = (uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)(v >> 32), j);
  return ((unsigned long long)hi << 32) | lo;
}

// This thread's share of rows [row0, row0 + 64) x columns [c0, c0 + 4 KS) of X:
// element e = tid + 256 i is row e / KS, columns 4 (e % KS) .. + 3.  Every load
// is unconditional from a clamped (always valid) address; zero past the row
// limit `hi` or past d.
template <int KS>
__device__ __forceinline__ void kn_fetch(f32x4 (&pre)[KS / 4], const float* __restrict__ X, int row0, int hi, int d,
                                         int c0, int vec, int tid) {
#pragma unroll
  for (int i = 0; i < KS / 4; ++i) {
    const int e = tid + KN_THREADS * i;
    const int r = row0 + e / KS, c = c0 + 4 * (e % KS);
    if (vec) {
      const bool ok = r < hi && c < d;
      f32x4 v = *reinterpret_cast<const f32x4*>(X + (ok ? (size_t)r * d + c : (size_t)0));
      pre[i] = ok ? v : f32x4{0.f, 0.f, 0.f, 0.f};
    } else {
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        const bool ok = r < hi && c + q < d;
        const float v = X[ok ? (size_t)r * d + c + q : (size_t)0];
        pre[i][q] = ok ? v : 0.f;
      }
    }
  }
}

template <int KS>
__device__ __forceinline__ void kn_put(float* __restrict__ Xs, const f32x4 (&pre)[KS / 4], int tid) {
  constexpr int S = kn_stride(KS);
#pragma unroll
  for (int i = 0; i < KS / 4; ++i) {
    const int e = tid + KN_THREADS * i;
    float* dst = Xs + (e / KS) * S + 4 * (e % KS);
    *reinterpret_cast<f32x2*>(dst) = f32x2{pre[i].x, pre[i].y};
    *reinterpret_cast<f32x2*>(dst + 2) = f32x2{pre[i].z, pre[i].w};
  }
}

// Stage query rows [row0, row0 + 128) x columns [c0, c0 + 4 KS) into LDS, zero past either edge.
template <int KS>
__device__ __forceinline__ void kn_stage_q(float* __restrict__ dst, const float* __restrict__ Q, long long row0,
                                           long long nq, int d, int c0, int vec, int tid) {
  constexpr int W = 4 * KS, S = kn_stride(KS);
  if (vec) {
    constexpr int W4 = W / 4;
#pragma unroll 4
    for (int e = tid; e < KN_QB * W4; e += KN_THREADS) {
      const int r = e / W4, c = 4 * (e % W4);
      const bool ok = row0 + r < nq && c0 + c < d;
      f32x4 v = *reinterpret_cast<const f32x4*>(Q + (ok ? (size_t)(row0 + r) * d + c0 + c : (size_t)0));
      if (!ok) v = f32x4{0.f, 0.f, 0.f, 0.f};
      *reinterpret_cast<f32x2*>(dst + r * S + c) = f32x2{v.x, v.y};
      *reinterpret_cast<f32x2*>(dst + r * S + c + 2) = f32x2{v.z, v.w};
    }
  } else {
#pragma unroll 4
    for (int e = tid; e < KN_QB * W; e += KN_THREADS) {
      const int r = e / W, c = e % W;
      const bool ok = row0 + r < nq && c0 + c < d;
      const float v = Q[ok ? (size_t)(row0 + r) * d + c0 + c : (size_t)0];
      dst[r * S + c] = ok ? v : 0.f;
    }
  }
}

// acc[s][t] += A_t (16 x 4 KS) * B_s (4 KS x 16); Xb = &Xs[col][g]
template <int KS>
__device__ __forceinline__ void kn_mma(const float* __restrict__ Xb, const float (&a)[2][KS], f32x4 (&acc)[4][2]) {
  constexpr int S = kn_stride(KS);
#pragma unroll
  for (int ks = 0; ks < KS; ++ks) {
#pragma unroll
    for (int s = 0; s < 4; ++s) {
      const float b = Xb[s * 16 * S + 4 * ks];
#pragma unroll
      for (int t = 0; t < 2; ++t) acc[s][t] = __builtin_amdgcn_mfma_f32_16x16x4f32(a[t][ks], b, acc[s][t], 0, 0, 0);
    }
  }
}

// The selection state of a workgroup in LDS; rows [32 w, 32 w + 32) belong to wave w alone.
struct KnSel {
  unsigned long long* list;  // [128][K] sorted keys
  unsigned long long* pend;  // [128][KN_PS]
  float* tau;                // [128] distance of the K-th key, NaN while the list has free slots
  unsigned* cnt;             // [128] pending keys
  int k;
};

// Merge the pending keys of query row q (c of them, 1 <= c <= KN_P) into its list; the whole wave.
__device__ __forceinline__ void kn_compact_one(const KnSel& L, int q, int c, int lane) {
  const int K = L.k;
  unsigned long long* lst = L.list + (size_t)q * K;
  const unsigned long long mine = lane < K ? lst[lane] : KN_FREE64;
  const unsigned long long pk = lane < c ? L.pend[q * KN_PS + lane] : KN_FREE64;
  int below = 0, prank = 0;  // pending keys above my list key; rank of my pending key
  for (int j = 0; j < c; ++j) {
    const unsigned long long pj = kn_bcast64(pk, j);
    const bool lt = mine < pj;
    const int nl = __popcll(__ballot(lt));       // list keys below p_j (free slots are never below)
    const int np = __popcll(__ballot(pk < pj));  // pending keys below p_j
    below += lt ? 1 : 0;
    if (lane == j) prank = nl + np;
  }
  const int lrank = lane + c - below;
  kn_wave_sync();  // every key is in registers
  if (lane < K && lrank < K) {
    lst[lrank] = mine;
    if (lrank == K - 1) L.tau[q] = mine == KN_FREE64 ? __builtin_nanf("") : __uint_as_float((uint32_t)(mine >> 32));
  }
  if (lane < c && prank < K) {
    lst[prank] = pk;
    if (prank == K - 1) L.tau[q] = __uint_as_float((uint32_t)(pk >> 32));
  }
  if (lane == 0) L.cnt[q] = 0;
}

// Compact every query of this wave that holds more than `over` pending keys; true if any did.
__device__ __forceinline__ bool kn_compact(const KnSel& L, int wave, int lane, unsigned over) {
  kn_wave_sync();
  const unsigned c = lane < 32 ? L.cnt[wave * 32 + lane] : 0u;
  unsigned long long todo = __ballot(c > over);
  if (todo == 0) return false;
  while (todo) {
    const int r = __builtin_ctzll(todo);
    todo &= todo - 1;
    int cr = __builtin_amdgcn_readlane((int)c, r);
    cr = cr > KN_P ? KN_P : cr;
    kn_compact_one(L, wave * 32 + r, cr, lane);
  }
  kn_wave_sync();
  return true;
}

template <int KS, bool MULTI>
__global__ __launch_bounds__(KN_THREADS) void knn_sweep_kernel(const KnArgs p) {
  constexpr int W = 4 * KS;  // floats of d per staged chunk
  constexpr int S = kn_stride(KS);
  extern __shared__ __attribute__((aligned(16))) unsigned char kn_lds[];
  float* Xs = reinterpret_cast<float*>(kn_lds);  // [64][S]  X tile (chunk)
  float* xnS = Xs + KN_XT * S;                   // [64]     |x|^2
  float* qnS = xnS + KN_XT;                      // [128]    |q|^2
  float* tauS = qnS + KN_QB;                     // [128]
  unsigned* cntS = reinterpret_cast<unsigned*>(tauS + KN_QB);  // [128]
  float* Qs = reinterpret_cast<float*>(cntS + KN_QB);          // [128][S]  Q tile (chunk)
  // the selection planes: behind the Q tile (d > 128), or in its bytes once the fragments are lifted
  unsigned long long* sel = reinterpret_cast<unsigned long long*>(MULTI ? Qs + KN_QB * S : Qs);

  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int col = lane & 15, g = lane >> 4;
  const int d = p.d, K = p.k;
  const long long q0 = (long long)blockIdx.x * KN_QB;
  const int nch = MULTI ? (d + W - 1) / W : 1;

  KnSel L;
  L.list = sel;
  L.pend = sel + (size_t)KN_QB * K;
  L.tau = tauS;
  L.cnt = cntS;
  L.k = K;

  // this workgroup's slab of X tiles
  const int ntiles = (p.n + KN_XT - 1) / KN_XT;
  const int per = ntiles / p.slabs, rem = ntiles % p.slabs, sb = blockIdx.y;
  const int t0 = sb * per + (sb < rem ? sb : rem), t1 = t0 + per + (sb < rem ? 1 : 0);
  const int hi = t1 * KN_XT < p.n ? t1 * KN_XT : p.n;  // row limit of the slab

  f32x4 pre[KS / 4];  // this thread's share of the next X tile (chunk)
  if (t0 < t1) kn_fetch<KS>(pre, p.X, t0 * KN_XT, hi, d, 0, p.vecx, tid);

  // prologue: |q|^2 (one chain per row over all columns) and, for d <= 128, the A fragments
  float a[2][KS];
  {
    float s = 0.f;
    for (int dc = 0; dc < nch; ++dc) {
      __syncthreads();
      kn_stage_q<KS>(Qs, p.Q, q0, p.nq, d, dc * W, p.vecq, tid);
      __syncthreads();
      if (tid < KN_QB) {
#pragma unroll 8
        for (int c = 0; c < W; ++c) {
          const float v = Qs[tid * S + c];
          s = fmaf(v, v, s);
        }
      }
      if (!MULTI) {
#pragma unroll
        for (int t = 0; t < 2; ++t)
#pragma unroll
          for (int ks = 0; ks < KS; ++ks) a[t][ks] = Qs[(wave * 32 + t * 16 + col) * S + 4 * ks + g];
      }
    }
    if (tid < KN_QB) qnS[tid] = s;
    __syncthreads();  // Q tile dead (d <= 128): its bytes become the selection planes
    for (int e = tid; e < KN_QB * K; e += KN_THREADS) L.list[e] = KN_FREE64;
    if (tid < KN_QB) {
      tauS[tid] = __builtin_nanf("");
      cntS[tid] = 0;
    }
    __syncthreads();
  }
  float qn[2][4], tau[2][4];
#pragma unroll
  for (int t = 0; t < 2; ++t)
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      qn[t][i] = qnS[wave * 32 + t * 16 + g * 4 + i];
      tau[t][i] = __builtin_nanf("");
    }

  const float* Xb = Xs + col * S + g;
  for (int tile = t0; tile < t1; ++tile) {
    f32x4 acc[4][2];
#pragma unroll
    for (int s = 0; s < 4; ++s)
#pragma unroll
      for (int t = 0; t < 2; ++t) acc[s][t] = f32x4{0.f, 0.f, 0.f, 0.f};

    for (int dc = 0; dc < nch; ++dc) {
      // (every reader of Xs / Qs of the step before passed the barrier that ended it)
      kn_put<KS>(Xs, pre, tid);
      if (MULTI) kn_stage_q<KS>(Qs, p.Q, q0, p.nq, d, dc * W, p.vecq, tid);
      __syncthreads();  // tile staged; on the first pass: lists, tau, counters initialised
      {  // |x|^2: 4 threads a row, thread r the columns c = r (mod 4)
        const int r = tid >> 2, qd = tid & 3;
        float s = 0.f;
#pragma unroll 8
        for (int i = 0; i < KS; ++i) {
          const float v = Xs[r * S + 4 * i + qd];
          s = fmaf(v, v, s);
        }
        s += __shfl_xor(s, 1);
        s += __shfl_xor(s, 2);
        if (qd == 0) xnS[r] = (MULTI && dc > 0) ? xnS[r] + s : s;
      }
      if (MULTI) {
#pragma unroll
        for (int t = 0; t < 2; ++t)
#pragma unroll
          for (int ks = 0; ks < KS; ++ks) a[t][ks] = Qs[(wave * 32 + t * 16 + col) * S + 4 * ks + g];
      }
      {  // the next step's X chunk: loads in flight behind the sweep below
        const bool wrap = dc + 1 == nch;
        const int nt = wrap ? tile + 1 : tile;
        if (nt < t1) kn_fetch<KS>(pre, p.X, nt * KN_XT, hi, d, wrap ? 0 : (dc + 1) * W, p.vecx, tid);
      }
      kn_mma<KS>(Xb, a, acc);
      __syncthreads();  // Xs / Qs free for the next step; xnS complete
    }

    // selection: wave-private from here to the next barrier
    const int j0 = tile * KN_XT + col;
#pragma unroll
    for (int s = 0; s < 4; ++s) {
      const float xn = xnS[s * 16 + col];
      const int j = j0 + s * 16;
      bool any = false;
#pragma unroll
      for (int t = 0; t < 2; ++t)
#pragma unroll
        for (int i = 0; i < 4; ++i) {
          const float raw = qn[t][i] + fmaf(-2.f, acc[s][t][i], xn);
          if (!(raw >= tau[t][i])) {  // below the K-th distance, or the list has free slots, or NaN
            const uint32_t hb = __float_as_uint(fmaxf(0.f, raw)) & 0x7FFFFFFFu;
            const int q = wave * 32 + t * 16 + g * 4 + i;
            const float tq = tauS[q];
            if (j < hi && !(__uint_as_float(hb) >= tq)) {
              const unsigned pos = atomicAdd(&cntS[q], 1u);
              if (pos < (unsigned)KN_P) L.pend[q * KN_PS + pos] = ((unsigned long long)hb << 32) | (uint32_t)j;
              any = true;
            }
          }
        }
      if (__ballot(any)) {
        if (kn_compact(L, wave, lane, KN_TRIG)) {
#pragma unroll
          for (int t = 0; t < 2; ++t)
#pragma unroll
            for (int i = 0; i < 4; ++i) tau[t][i] = tauS[wave * 32 + t * 16 + g * 4 + i];
        }
      }
    }
  }

  kn_compact(L, wave, lane, 0u);
  __syncthreads();
  unsigned long long* out = p.ws + ((size_t)blockIdx.y * (size_t)p.nq + (size_t)q0) * K;
  const long long rows = p.nq - q0 < KN_QB ? p.nq - q0 : KN_QB;
  for (int e = tid; e < (int)rows * K; e += KN_THREADS) out[e] = L.list[e];
}

// ---- merge -------------------------------------------------------------------------

struct KnMerge {
  const float* da;                // running state A (may be the output)
  const long long* ia;
  const float* db;                // state B or null
  const long long* ib;
  const unsigned long long* ws;   // [S][nq][K] keys or null
  float* dout;
  long long* iout;
  long long nq, base;
  int k, slabs;
};

__device__ __forceinline__ bool kn_less(uint32_t ha, long long ia, uint32_t hb, long long ib) {
  return ha < hb || (ha == hb && ia < ib);
}

__device__ __forceinline__ long long kn_bcast_i64(long long v, int j) { return (long long)kn_bcast64((unsigned long long)v, j); }

__global__ __launch_bounds__(KN_THREADS) void knn_merge_kernel(const KnMerge p) {
  __shared__ uint32_t mh[4][64];
  __shared__ long long mi[4][64];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int K = p.k;
  const long long qraw = (long long)blockIdx.x * 4 + wave;
  const bool live = qraw < p.nq;
  const long long q = live ? qraw : p.nq - 1;  // a spare wave repeats the last query and writes nothing
  const bool in = lane < K;

  uint32_t ch = KN_FREE;
  long long ci = -1;
  if (in) {
    ci = p.ia[q * K + lane];
    ch = ci < 0 ? KN_FREE : (__float_as_uint(p.da[q * K + lane]) & 0x7FFFFFFFu);
    ci = ci < 0 ? -1 : ci;
  }
  const int lists = (p.db ? 1 : 0) + p.slabs;
  for (int l = 0; l < lists; ++l) {
    uint32_t nh = KN_FREE;
    long long ni = -1;
    if (in) {
      if (p.db && l == 0) {
        ni = p.ib[q * K + lane];
        nh = ni < 0 ? KN_FREE : (__float_as_uint(p.db[q * K + lane]) & 0x7FFFFFFFu);
        ni = ni < 0 ? -1 : ni;
      } else {
        const int s = l - (p.db ? 1 : 0);
        const unsigned long long key = p.ws[((size_t)s * (size_t)p.nq + (size_t)q) * K + lane];
        nh = (uint32_t)(key >> 32);
        ni = key == KN_FREE64 ? -1 : p.base + (long long)(uint32_t)key;
        nh = key == KN_FREE64 ? KN_FREE : nh;
      }
    }
    int rc = lane, rn = lane;  // ranks of my current / my incoming entry in the union
    for (int j = 0; j < K; ++j) {
      const uint32_t bh = (uint32_t)__builtin_amdgcn_readlane((int)nh, j);
      const long long bi = kn_bcast_i64(ni, j);
      const uint32_t ah = (uint32_t)__builtin_amdgcn_readlane((int)ch, j);
      const long long ai = kn_bcast_i64(ci, j);
      rc += kn_less(bh, bi, ch, ci) ? 1 : 0;   // incoming strictly below mine
      rn += kn_less(nh, ni, ah, ai) ? 0 : 1;   // current at or below my incoming: a tie keeps the current first
    }
    __syncthreads();
    if (in && rc < K) {
      mh[wave][rc] = ch;
      mi[wave][rc] = ci;
    }
    if (in && rn < K) {
      mh[wave][rn] = nh;
      mi[wave][rn] = ni;
    }
    __syncthreads();
    if (in) {
      ch = mh[wave][lane];
      ci = mi[wave][lane];
    }
  }
  if (live && in) {
    p.dout[q * K + lane] = ch == KN_FREE ? INFINITY : __uint_as_float(ch);
    p.iout[q * K + lane] = ch == KN_FREE ? -1 : ci;
  }
}

// ---- host side ---------------------------------------------------------------------

template <int KS, bool MULTI>
int kn_launch(const KnArgs& a, hipStream_t s) {
  const size_t lds = kn_lds_bytes(KS, MULTI, a.k);
  if (lds > (size_t)KN_LDS_MAX) return -3;
  static bool allowed = false;  // the dynamic LDS above 64 KiB must be allowed once
  if (!allowed) {
    if (hipFuncSetAttribute((const void*)knn_sweep_kernel<KS, MULTI>, hipFuncAttributeMaxDynamicSharedMemorySize,
                            (int)kn_lds_bytes(KS, MULTI, KN_MAXK)) != hipSuccess) {
      (void)hipGetLastError();
      return -4;
    }
    allowed = true;
  }
  const dim3 grid((unsigned)((a.nq + KN_QB - 1) / KN_QB), (unsigned)a.slabs);
  hipLaunchKernelGGL((knn_sweep_kernel<KS, MULTI>), grid, dim3(KN_THREADS), lds, s, a);
  const int rc = (int)hipGetLastError();
  return rc ? -100 - rc : 0;
}

int kn_merge_launch(const KnMerge& m, hipStream_t s) {
  if (m.nq == 0) return 0;
  hipLaunchKernelGGL(knn_merge_kernel, dim3((unsigned)((m.nq + 3) / 4)), dim3(KN_THREADS), 0, s, m);
  const int rc = (int)hipGetLastError();
  return rc ? -100 - rc : 0;
}

bool kn_shape_ok(long long nq, int k) { return nq >= 0 && nq <= 0x7FFFFFFFll * 4 && k >= 1 && k <= KN_MAXK; }

}  // namespace

extern "C" {

// Bytes of workspace a search over `slabs` slabs needs: u64 keys [slabs][q][k]; 0 outside the ranges.
unsigned long long mr_knn_workspace_bytes(long long q, int k, int slabs) {
  if (!kn_shape_ok(q, k) || slabs < 1 || slabs > KN_MAXS) return 0;
  return 8ull * (unsigned long long)slabs * (unsigned long long)q * (unsigned long long)k;
}

// Fold the rows of X [n, d] (indices base + j) into the running lists dist fp32 [nq, k] / idx int64 [nq, k] of
// the queries Q [nq, d] (see the header).  workspace: mr_knn_workspace_bytes(nq, k, slabs) bytes.
// -2: a shape outside 1 <= d <= 512, 1 <= k <= 64, nq >= 0, 0 <= n < 2^31, 1 <= slabs <= 65535, or base + n
// leaves int64;  -3: LDS too small;  -4: the dynamic-LDS attribute was refused;  <= -100: -100 - the launch's
// HIP error.
int mr_knn_search(const void* Q, const void* X, long long nq, long long n, int d, int k, long long base, int slabs,
                  void* workspace, void* dist, void* idx, hipStream_t s) {
  if (!kn_shape_ok(nq, k) || d < 1 || d > KN_MAXD || n < 0 || n > 0x7FFFFFFFll || slabs < 1 || slabs > KN_MAXS ||
      base < 0 || base > INT64_MAX - n)
    return -2;
  if (nq == 0) return 0;
  const long long ntiles = (n + KN_XT - 1) / KN_XT;
  const int S = n == 0 ? 0 : (int)(slabs < ntiles ? slabs : ntiles);  // no slab without a tile
  if (S > 0) {
    KnArgs a;
    a.Q = (const float*)Q;
    a.X = (const float*)X;
    a.ws = (unsigned long long*)workspace;
    a.nq = nq;
    a.n = (int)n;
    a.d = d;
    a.k = k;
    a.slabs = S;
    a.vecq = (d % 4 == 0 && ((uintptr_t)Q & 15) == 0) ? 1 : 0;
    a.vecx = (d % 4 == 0 && ((uintptr_t)X & 15) == 0) ? 1 : 0;
    const int rc = d > 128  ? kn_launch<16, true>(a, s)
                   : d > 64 ? kn_launch<32, false>(a, s)
                   : d > 16 ? kn_launch<16, false>(a, s)
                            : kn_launch<4, false>(a, s);
    if (rc) return rc;
  }
  KnMerge m;
  m.da = (const float*)dist;
  m.ia = (const long long*)idx;
  m.db = nullptr;
  m.ib = nullptr;
  m.ws = (const unsigned long long*)workspace;
  m.dout = (float*)dist;
  m.iout = (long long*)idx;
  m.nq = nq;
  m.base = base;
  m.k = k;
  m.slabs = S;
  return kn_merge_launch(m, s);
}

// out = the k smallest (dist, idx) pairs of two running states; out may be either input.
int mr_knn_merge(const void* dist_a, const void* idx_a, const void* dist_b, const void* idx_b, long long nq, int k,
                 void* dist_out, void* idx_out, hipStream_t s) {
  if (!kn_shape_ok(nq, k)) return -2;
  KnMerge m;
  m.da = (const float*)dist_a;
  m.ia = (const long long*)idx_a;
  m.db = (const float*)dist_b;
  m.ib = (const long long*)idx_b;
  m.ws = nullptr;
  m.dout = (float*)dist_out;
  m.iout = (long long*)idx_out;
  m.nq = nq;
  m.base = 0;
  m.k = k;
  m.slabs = 0;
  return kn_merge_launch(m, s);
}

}  // extern "C"
