// segsort.hip — segmented merge sort of CSR value lists, and the multi-quantile
// pick over the sorted lists (ops/segments.py: sort, unique, topk, quantiles).
//
// A rank's value lists are one CSR pair off[m + 1] / val[n] (segments.hip).
// Every list is sorted in place (lists do not move), 64-bit values as the
// unsigned order key of ops/segments.order_key: int64 with the sign bit
// flipped, float64 bits flipped so that -0.0 < +0.0 and NaNs order by their
// bits; `descending` complements the key.  Buffers always hold raw values: the
// key transform is applied on load and inverted on store, so every bit pattern
// (NaN payloads, -0.0) round-trips.
//
// The work is split by VALUES, not keys: aligned tiles of T = 256 x 8 values,
// one workgroup each, whatever the list lengths.  No host sync, no look-back.
//
// Phase A (seg_block_sort_kernel).  A workgroup finds its tile's first and last
// list by two wavefront-wide searches in off[] (64 probes per step: 3-4 steps
// of one memory round trip each for a million lists, not 20), gives every value
// a tile-local list id (the tile offset of its list's head: non-decreasing
// along the tile), and sorts (id, key) with a bitonic network: a thread holds
// 8 consecutive elements, so the strides 4, 2, 1 of every merge step run in
// registers and only strides >= 8 go through LDS (36 LDS stages instead of 66
// for T = 2048; 24 KB of LDS, so six workgroups fit a CU).  Lists lying inside
// the tile are finished and go to `out`.
//
// Phase B (seg_merge_kernel, one launch per pass).  A list crossing tile
// boundaries is a row of sorted pieces, numbered from 0 at the list's own first
// tile.  Pass p merges, inside each list, the runs of pieces [2j 2^p, (2j+1) 2^p)
// and [(2j+1) 2^p, (2j+2) 2^p); a run without a right neighbour is NOT copied.
// Grid: one workgroup per output tile; at most two merging lists touch a tile
// (the ones holding its first and its last value).  For each the workgroup
// finds its slice of the run pair by two merge-path diagonal searches (again
// wavefront-wide, two wavefronts side by side), stages the <= T inputs in LDS,
// ranks every staged element in the other side by binary search in LDS (ties:
// left run first), scatters to a second LDS array and writes coalesced.
//
// Ping-pong between `out` and `tmp`.  Deviations from a per-list parity and a
// sequential per-thread merge, both for correctness / simplicity:
//   * the buffer is chosen per PIECE, not per list: a piece is written by
//     phase A to the buffer whose index is the parity of the number of merges
//     still ahead of it (merges_from).  All pieces of a run pair share their
//     future, so both inputs of a merge lie in one buffer and its output goes
//     to the other, and every piece ends in `out`.  With one parity per list an
//     unmerged tail run (3 pieces: pass 1 reads piece 2 from the buffer it
//     writes) would be overwritten while it is read;
//   * the in-LDS merge is rank-and-scatter instead of a per-thread sequential
//     merge: no second per-thread diagonal search, no divergent loop.
// The host launches ceil(log2(ceil(n / T) + 1)) passes, from n alone; a
// workgroup with nothing to merge exits after its two searches.
//
// Offsets are clamped to [0, n] as they are read, so a malformed off[] gives a
// wrong order but never an access outside val / out / tmp.
#include <hip/hip_runtime.h>
#include "mr_common.h"

namespace mr {
namespace segsort {

constexpr int THREADS = 256;
constexpr int V = 8;               // values per thread (register-resident bitonic strides 4, 2, 1)
constexpr int T = THREADS * V;     // values per tile
constexpr u64 SIGN = 1ull << 63;
constexpr int PICK_MAXQ = 16;      // quantiles per mr_seg_pick launch (kernel-argument array)

__device__ __forceinline__ u64 to_key(u64 b, int isf, int desc) {
  const u64 k = (isf && (b & SIGN)) ? ~b : b ^ SIGN;
  return desc ? ~k : k;
}
__device__ __forceinline__ u64 from_key(u64 k, int isf, int desc) {
  if (desc) k = ~k;
  return (isf && !(k & SIGN)) ? ~k : k ^ SIGN;
}

__device__ __forceinline__ long long ld_off(const long long* __restrict__ off, long long s, long long n) {
  const long long v = off[s];
  return v < 0 ? 0 : (v > n ? n : v);
}

// Smallest x in [lo, hi] at which pred is false (pred: true on a prefix of
// [lo, hi), never evaluated at hi).  Called by a whole wavefront with equal
// lo / hi: 64 probes per step.
template <typename F>
__device__ __forceinline__ long long wave_partition(long long lo, long long hi, F pred) {
  const int lane = threadIdx.x & 63;
  while (lo < hi) {
    const long long step = (hi - lo + 63) >> 6;
    const long long x = lo + lane * step;
    const bool t = x < hi && pred(x);
    const int nt = __popcll(__ballot(t));
    if (nt == 0) break;
    const long long nhi = lo + nt * step;
    lo += (nt - 1) * step + 1;
    if (nhi < hi) hi = nhi;
  }
  return lo;
}

// list holding value i: largest s in [0, m - 1] with off[s] <= i
__device__ __forceinline__ long long wave_seg_of(const long long* __restrict__ off, long long m, long long n,
                                                 long long i) {
  return wave_partition(1, m, [&](long long s) { return ld_off(off, s, n) <= i; }) - 1;
}

// largest s in [lo, hi] with off[s] <= i (off[lo] <= i), one thread
__device__ __forceinline__ long long seg_of(const long long* __restrict__ off, long long n, long long lo, long long hi,
                                            long long i) {
  while (lo < hi) {
    const long long mid = (lo + hi + 1) >> 1;
    if (ld_off(off, mid, n) <= i) lo = mid;
    else hi = mid - 1;
  }
  return lo;
}

// Piece k of a list of c pieces is merged in pass q iff its run pair has a
// right run: first piece of the pair + 2^q < c.
__device__ __forceinline__ bool merged_in(long long k, long long c, int q) {
  return (((k >> (q + 1)) << (q + 1)) + (1ll << q)) < c;
}
// merges ahead of piece k from pass q on (passes exist while 2^q < c)
__device__ __forceinline__ int merges_from(long long k, long long c, int q) {
  int r = 0;
  for (; q < 62 && (1ll << q) < c; ++q) r += merged_in(k, c, q) ? 1 : 0;
  return r;
}

__device__ __forceinline__ void cswap(u64& ka, u32& la, u64& kb, u32& lb, bool up) {
  const bool gt = la > lb || (la == lb && ka > kb);
  if (gt == up) {
    const u64 k = ka; ka = kb; kb = k;
    const u32 l = la; la = lb; lb = l;
  }
}

// bitonic stride J < V inside a thread's V consecutive elements (base = index
// of its first element; kk = size of the sorted runs being built)
template <int J>
__device__ __forceinline__ void reg_stage(u64 (&k)[V], u32 (&l)[V], int base, int kk) {
#pragma unroll
  for (int r = 0; r < V; ++r)
    if ((r & J) == 0) cswap(k[r], l[r], k[r | J], l[r | J], ((base + r) & kk) == 0);
}

__global__ void __launch_bounds__(THREADS) seg_block_sort_kernel(const long long* __restrict__ off, long long m,
                                                                 const u64* __restrict__ val, long long n, int isf,
                                                                 int desc, u64* __restrict__ out,
                                                                 u64* __restrict__ tmp) {
  __shared__ u64 s_key[T];
  __shared__ u32 s_lid[T];
  __shared__ long long s_seg[2];
  __shared__ int s_par[2];   // buffer (0 out, 1 tmp) of the tile's first / last list
  __shared__ u32 s_lidb;     // local id of the tile's last list
  const int tid = threadIdx.x, wave = tid >> 6;
  const long long t = blockIdx.x, tile0 = t * T;
  const int cnt = n - tile0 < T ? (int)(n - tile0) : T;
  if (wave < 2) {
    const long long s = wave_seg_of(off, m, n, wave == 0 ? tile0 : tile0 + cnt - 1);
    if ((tid & 63) == 0) {
      const long long b = ld_off(off, s, n), e = ld_off(off, s + 1, n);
      const long long f = b / T, c = e > b ? (e - 1) / T - f + 1 : 0;
      s_seg[wave] = s;
      s_par[wave] = (c > 1 && t >= f) ? (merges_from(t - f, c, 0) & 1) : 0;
      if (wave == 1) s_lidb = b > tile0 ? (u32)(b - tile0) : 0u;
    }
  }
  __syncthreads();
  const long long sa = s_seg[0], sb = s_seg[1];

  u64 k[V];
  u32 l[V];
  const int base = tid * V;
  {
    const long long i0 = tile0 + base;
    long long s = sa, e = 0;
    u32 lid = 0;
    if (i0 < n) {
      s = seg_of(off, n, sa, sb > sa ? sb : sa, i0);
      const long long b = ld_off(off, s, n);
      e = ld_off(off, s + 1, n);
      lid = b > tile0 ? (u32)(b - tile0) : 0u;
    }
#pragma unroll
    for (int r = 0; r < V; ++r) {
      const long long i = i0 + r;
      if (i < n) {
        if (i >= e && s < sb) {  // next non-empty list: the one holding value i
          s = ld_off(off, s + 2, n) > i ? s + 1 : seg_of(off, n, s + 1, sb, i);
          const long long b = ld_off(off, s, n);
          e = ld_off(off, s + 1, n);
          lid = b > tile0 ? (u32)(b - tile0) : 0u;
        }
        k[r] = to_key(val[i], isf, desc);
        l[r] = lid;
      } else {
        k[r] = ~0ull;  // padding sorts behind every list
        l[r] = (u32)T;
      }
    }
  }
  reg_stage<1>(k, l, base, 2);
  reg_stage<2>(k, l, base, 4);
  reg_stage<1>(k, l, base, 4);
  reg_stage<4>(k, l, base, 8);
  reg_stage<2>(k, l, base, 8);
  reg_stage<1>(k, l, base, 8);
  for (int kk = 2 * V; kk <= T; kk <<= 1) {
#pragma unroll
    for (int r = 0; r < V; ++r) {
      s_key[base + r] = k[r];
      s_lid[base + r] = l[r];
    }
    __syncthreads();
    for (int j = kk >> 1; j >= V; j >>= 1) {
#pragma unroll
      for (int u = 0; u < V / 2; ++u) {
        const int p = tid + u * THREADS;
        const int i = ((p & ~(j - 1)) << 1) | (p & (j - 1));
        const int h = i | j;
        u64 ka = s_key[i], kb = s_key[h];
        u32 la = s_lid[i], lb = s_lid[h];
        const bool gt = la > lb || (la == lb && ka > kb);
        if (gt == ((i & kk) == 0)) {
          s_key[i] = kb; s_key[h] = ka;
          s_lid[i] = lb; s_lid[h] = la;
        }
      }
      __syncthreads();
    }
#pragma unroll
    for (int r = 0; r < V; ++r) {
      k[r] = s_key[base + r];
      l[r] = s_lid[base + r];
    }
    reg_stage<4>(k, l, base, kk);
    reg_stage<2>(k, l, base, kk);
    reg_stage<1>(k, l, base, kk);
  }
  // (every thread's last LDS reads were of its own V slots: no barrier needed before it rewrites them)
#pragma unroll
  for (int r = 0; r < V; ++r) {
    s_key[base + r] = k[r];
    s_lid[base + r] = l[r];
  }
  __syncthreads();
  const u32 lidb = s_lidb;
  const int par_a = s_par[0], par_b = s_par[1];
#pragma unroll
  for (int u = 0; u < V; ++u) {
    const int i = tid + u * THREADS;
    if (i < cnt) {
      const u32 lid = s_lid[i];
      const int par = lid == 0 ? par_a : (lid == lidb ? par_b : 0);
      (par ? tmp : out)[tile0 + i] = from_key(s_key[i], isf, desc);
    }
  }
}

struct MergeJob {
  long long A0, B0, B1;  // left run [A0, B0), right run [B0, B1)
  long long o0, o1;      // this tile's output positions of the pair
  int src;               // buffer holding both runs (0 out, 1 tmp); the output goes to the other
  int active;
};

__global__ void __launch_bounds__(THREADS) seg_merge_kernel(const long long* __restrict__ off, long long m,
                                                            long long n, int q, int isf, int desc, u64* out,
                                                            u64* tmp) {
  __shared__ u64 s_in[T];
  __shared__ u64 s_out[T];
  __shared__ long long s_seg[2];
  __shared__ MergeJob s_job[2];
  __shared__ long long s_split[2];
  const int tid = threadIdx.x, wave = tid >> 6;
  const long long t = blockIdx.x, tile0 = t * T;
  const long long tile1 = tile0 + T < n ? tile0 + T : n;
  if (wave < 2) {
    const long long s = wave_seg_of(off, m, n, wave == 0 ? tile0 : tile1 - 1);
    if ((tid & 63) == 0) {
      MergeJob J;
      J.active = 0;
      const long long b = ld_off(off, s, n), e = ld_off(off, s + 1, n);
      if (e > b) {
        const long long f = b / T, c = (e - 1) / T - f + 1, k = t - f;
        if (k >= 0 && k < c && merged_in(k, c, q)) {
          const long long j2 = (k >> (q + 1)) << (q + 1);  // first piece of the run pair
          const long long a0 = (f + j2) * T, b1 = (f + j2 + (2ll << q)) * T;
          J.A0 = b > a0 ? b : a0;
          J.B0 = (f + j2 + (1ll << q)) * T;
          J.B1 = e < b1 ? e : b1;
          J.o0 = b > tile0 ? b : tile0;
          J.o1 = e < tile1 ? e : tile1;
          J.src = merges_from(k, c, q) & 1;
          J.active = J.A0 < J.B0 && J.B0 < J.B1 && J.A0 <= J.o0 && J.o0 < J.o1 && J.o1 <= J.B1;
        }
      }
      s_seg[wave] = s;
      s_job[wave] = J;
    }
  }
  __syncthreads();
  const bool act[2] = {s_job[0].active != 0, s_job[1].active != 0 && s_seg[1] != s_seg[0]};
  if (!act[0] && !act[1]) return;
  for (int L = 0; L < 2; ++L) {
    if (!act[L]) continue;
    const MergeJob J = s_job[L];
    const u64* src = J.src ? tmp : out;
    u64* dst = J.src ? out : tmp;
    const long long lenA = J.B0 - J.A0, lenB = J.B1 - J.B0;
    if (wave < 2) {
      // merge-path split of diagonal d: elements taken from the left run among the first d outputs
      const long long d = (wave == 0 ? J.o0 : J.o1) - J.A0;
      const long long a = wave_partition(d > lenB ? d - lenB : 0, d < lenA ? d : lenA, [&](long long x) {
        return to_key(src[J.A0 + x], isf, desc) <= to_key(src[J.B0 + d - 1 - x], isf, desc);
      });
      if ((tid & 63) == 0) s_split[wave] = a;
    }
    __syncthreads();
    const long long a0 = s_split[0], a1 = s_split[1], b0 = (J.o0 - J.A0) - a0;
    const int total = (int)(J.o1 - J.o0);
    const int na = (int)(a1 - a0), nb = total - na;
    if (na >= 0 && nb >= 0) {  // (always, for sorted runs)
      for (int i = tid; i < total; i += THREADS)
        s_in[i] = to_key(src[i < na ? J.A0 + a0 + i : J.B0 + b0 + (i - na)], isf, desc);
      __syncthreads();
      for (int i = tid; i < total; i += THREADS) {
        const u64 x = s_in[i];
        int lo, hi;
        if (i < na) {  // left element: behind the right elements smaller than it
          lo = na; hi = total;
          while (lo < hi) {
            const int mid = (lo + hi) >> 1;
            if (s_in[mid] < x) lo = mid + 1;
            else hi = mid;
          }
          s_out[i + lo - na] = x;
        } else {       // right element: behind the left elements not larger than it
          lo = 0; hi = na;
          while (lo < hi) {
            const int mid = (lo + hi) >> 1;
            if (s_in[mid] <= x) lo = mid + 1;
            else hi = mid;
          }
          s_out[i - na + lo] = x;
        }
      }
      __syncthreads();
      for (int i = tid; i < total; i += THREADS) dst[J.o0 + i] = from_key(s_out[i], isf, desc);
    }
    __syncthreads();  // s_in / s_split are reused by the second list
  }
}

struct PickQs {
  double q[PICK_MAXQ];
};

// One thread per (list, q): linear interpolation between the two sorted
// values around (len - 1) q.  Every operation is rounded on its own (the CPU
// specification of ops/segments.quantiles rounds twice): contraction into FMAs
// is switched off for the kernel's own operators (the __dmul_rn / __dadd_rn
// wrappers are inlined with their header's contraction setting and do fuse).
template <typename VT>
__global__ void __launch_bounds__(256) seg_pick_kernel(const long long* __restrict__ off, long long m,
                                                       const VT* __restrict__ sv, long long n, PickQs qs, int k,
                                                       int col0, int ld, double* __restrict__ out) {
#pragma clang fp contract(off)
  const long long g = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (g >= m * k) return;
  const long long s = g / k;
  const int j = (int)(g - s * k);
  const long long b = ld_off(off, s, n), e = ld_off(off, s + 1, n);
  double r = __builtin_nan("");
  if (e > b) {
    const double pos = (double)(e - b - 1) * qs.q[j];
    const double fl = floor(pos), ce = ceil(pos);
    long long lo = (long long)fl, hi = (long long)ce;
    lo = lo < 0 ? 0 : (lo > e - b - 1 ? e - b - 1 : lo);
    hi = hi < 0 ? 0 : (hi > e - b - 1 ? e - b - 1 : hi);
    const double x = (double)sv[b + lo], y = (double)sv[b + hi];
    r = x + (y - x) * (pos - fl);
  }
  out[s * ld + col0 + j] = r;
}

}  // namespace segsort
}  // namespace mr

extern "C" {

int mr_seg_sort_tile(void) { return mr::segsort::T; }

// out[off[s] .. off[s+1]) = val[off[s] .. off[s+1]) sorted, for every s < m.
// off: int64[m + 1], off[0] == 0, off[m] == n, non-decreasing.  vtype: 0 int64,
// 1 float64.  out, tmp: n words each, neither aliasing val.
int mr_seg_sort(const void* off, unsigned long long m, const void* val, unsigned long long n, int vtype,
                int descending, void* out, void* tmp, hipStream_t stream) {
  using namespace mr::segsort;
  if (n == 0 || m == 0) return 0;
  if (vtype < 0 || vtype > 1 || !out || !tmp) return -1;
  const unsigned long long tiles = (n + T - 1) / T;
  if (tiles > 0x7FFFFFFFull) return -1;
  hipLaunchKernelGGL(seg_block_sort_kernel, dim3((unsigned)tiles), dim3(THREADS), 0, stream, (const long long*)off,
                     (long long)m, (const u64*)val, (long long)n, vtype, descending ? 1 : 0, (u64*)out, (u64*)tmp);
  // a list of n values has at most tiles + 1 pieces
  for (int q = 0; (1ull << q) < tiles + 1; ++q)
    hipLaunchKernelGGL(seg_merge_kernel, dim3((unsigned)tiles), dim3(THREADS), 0, stream, (const long long*)off,
                       (long long)m, (long long)n, q, vtype, descending ? 1 : 0, (u64*)out, (u64*)tmp);
  return (int)hipGetLastError();
}

// out[s, j] (float64, m rows of k) = the qs[j]-quantile of the SORTED list s of
// sv (vtype as above; int64 values are converted to float64), NaN for an empty
// list.  qs: k doubles in host memory (read before the call returns).
int mr_seg_pick(const void* off, unsigned long long m, const void* sv, unsigned long long n, int vtype,
                const double* qs, int k, void* out, hipStream_t stream) {
  using namespace mr::segsort;
  if (m == 0 || k <= 0) return 0;
  if (vtype < 0 || vtype > 1 || !qs || !out) return -1;
  for (int c0 = 0; c0 < k; c0 += PICK_MAXQ) {
    PickQs Q;
    const int kc = k - c0 < PICK_MAXQ ? k - c0 : PICK_MAXQ;
    for (int j = 0; j < PICK_MAXQ; ++j) Q.q[j] = j < kc ? qs[c0 + j] : 0.0;
    const unsigned long long blocks = (m * (unsigned long long)kc + 255) / 256;
    if (blocks > 0x7FFFFFFFull) return -1;
    if (vtype == 0)
      hipLaunchKernelGGL(seg_pick_kernel<long long>, dim3((unsigned)blocks), dim3(256), 0, stream,
                         (const long long*)off, (long long)m, (const long long*)sv, (long long)n, Q, kc, c0, k,
                         (double*)out);
    else
      hipLaunchKernelGGL(seg_pick_kernel<double>, dim3((unsigned)blocks), dim3(256), 0, stream,
                         (const long long*)off, (long long)m, (const double*)sv, (long long)n, Q, kc, c0, k,
                         (double*)out);
  }
  return (int)hipGetLastError();
}

}  // extern "C"
