// kmeans_bf16.hip — the k-means map step of kmeans.hip for bf16 points, on
// the 16-bit matrix cores, with the fp32 centroids split into bf16 pieces.
//
//   C_T        = sum of the first T bf16 pieces of C          (T = terms, 1..3)
//   labels[i]  = argmin_j  |C_T[j]|^2 - 2 x_i . C_T[j]         (lowest j on ties)
//   sums / counts / cost : as kmeans.hip (float64 / int64 / float64, added into)
//
// X [n, d] is bf16 row-major, C [k, d] fp32; 1 <= d <= 512, 1 <= k <= 4096.
// A bf16 x bf16 product is exact in fp32, so x . C_T is T bf16 MFMA chains
// into ONE fp32 accumulator, and with T = 3 the pieces carry every mantissa
// bit of an fp32 centroid.  Non-finite coordinates are unspecified (labels
// stay inside [0, k), nothing is indexed out of bounds).
//
// Two launches per step, no host synchronisation, no allocation.
//
// 1. Prologue (kmeans_bf16_split_kernel, one wave per centroid): piece t =
//    bf16_rne(c - sum of the pieces before it), the residual formed in fp32
//    (exact), and cn[j] = fl32(|C_T[j]|^2) as ONE length-d fp32 fma chain in
//    column order.  It writes the whole workspace, padding included, so the
//    workspace needs no clearing:
//      planes  bf16 [T][kpad][wd]   kpad = k rounded up to 64, wd = d rounded
//                                   up to 32; zero past k and past d
//      cn      fp32 [kpad]          +inf past k, so a padding centroid never wins
//    (mr_kmeans_bf16_workspace_bytes = 2 T kpad wd + 4 kpad).
//
// 2. Main kernel.  A workgroup is 4 waves and owns a super-tile of 64 PT
//    points: wave w owns PT 16-point MFMA tiles, the M dimension of
//    __builtin_amdgcn_mfma_f32_16x16x32_bf16.  Workgroups are persistent.
//
//   * LDS is addressed in 16-byte slots (8 bf16).  A row of 32 KS bf16 takes
//     4 KS slots and has a stride of S = 4 KS + 1 slots.  The super-tile's
//     points are staged once (16-byte loads when d % 8 == 0 and X is aligned,
//     zero past n and past d) and stay for the accumulation; each lane lifts
//     its A fragments, a[tile][ks] = slot 4 ks + (lane >> 4) of row lane & 15
//     (8 consecutive k at 8 (lane >> 4)), into registers, 4 VGPRs each, for
//     the whole centroid sweep.  The register budget of 64 VGPRs of A is
//     spent on point tiles while d is small (one B read feeds PT MFMAs) and
//     on d beyond that, so no d is chunked:
//       d <= 32: KS 1, PT 4   d <= 64: KS 2, PT 4   d <= 128: KS 4, PT 2
//       d <= 256: KS 8, PT 2  d <= 512: KS 16, PT 1
//   * Centroid tiles of CT = 16 NS columns are copied from the workspace as T
//     piece planes [T][CT][S] with their cn: no split, no squares here.  A
//     B-fragment read is one 16-byte read of slot col * S + 4 ks + g
//     (col = lane & 15, g = lane >> 4), i.e. the four banks
//     4 (col (4 KS + 1) + g + 4 ks) .. + 3  (mod 32).  A 16-byte read is
//     served 8 lanes a cycle (8 x 4 banks = 32); those are 8 consecutive
//     col of one g, and col (4 KS + 1) mod 8 = col (KS even) or 5 col (KS = 1),
//     distinct over 8 consecutive col: no bank is asked twice.  Were a cycle
//     to serve 16 lanes on 64 banks, col (4 KS + 1) mod 16 is col, 5 col or
//     9 col: distinct again.  The A-fragment reads have the same pattern.
//   * Per k-step and piece, one B read per column tile feeds PT MFMAs.  A
//     tile's columns are swept two column tiles at a time (a rolled loop, so
//     the live B fragments and accumulators leave room for a second wave):
//     2 x PT independent accumulator chains, and the T pieces of a k-step go
//     into the same accumulator.  score = fmaf(-2, acc, cn).
//   * Argmin, the xor-shuffle reduce, the clamp, the cost and the three
//     accumulation modes are kmeans.hip's; the rows added are the bf16 rows in
//     LDS, widened by a shift.
//
// Compiler resource report (gfx950, -O3, -Rpass-analysis=kernel-resource-usage;
// no scratch in any of the 15 variants; LDS is all dynamic: the tiles below,
// plus mode 1's 4 k (d + 1) bytes).  Registers are the T = 3 figures (T = 1, 2
// take no more); waves/SIMD is what the registers allow (the kernel asks for
// two with amdgpu_waves_per_eu where the LDS lets two workgroups share a CU),
// workgroups/CU what LDS and registers allow together with mode 0 or a small k:
//   variant (d)             VGPRs  AGPRs  waves/SIMD  tile LDS, T = 1 / 2 / 3 (bytes)  workgroups/CU
//   KS 1  PT 4 NS 4 (<= 32)   209      0      2         28 928 /  34 048 /  39 168         2
//   KS 2  PT 4 NS 4 (<= 64)   255      0      2         49 408 /  58 624 /  67 840         2
//   KS 4  PT 2 NS 2 (<= 128)  163      0      3         45 184 /  53 888 /  62 592         2
//   KS 8  PT 2 NS 2 (<= 256)  255     16      1         86 144 / 103 040 / 119 936         1
//   KS 16 PT 1 NS 1 (<= 512)  171      4      2         84 032 / 100 672 / 117 312         1
// At d = 128 the tiles take 62 592 bytes at T = 3: two workgroups per CU, two
// waves per SIMD, where kmeans.hip's 101 632 bytes leave one.  The launcher
// sizes the persistent grid for at most two workgroups per CU.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef unsigned u32x4 __attribute__((ext_vector_type(4)));
typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));

namespace {

constexpr int KB_THREADS = 256;  // 4 waves
constexpr int KB_MAXD = 512, KB_MAXK = 4096;
constexpr int KB_LDS_MAX = 160 * 1024;
constexpr int KB_KPAD = 64;  // the workspace pads k to this; every CT divides it

struct KbArgs {
  const uint16_t* X;  // bf16 bits
  const u32x4* P;     // workspace: piece planes [T][kpad][wd8] slots
  const float* cn;    // workspace: [kpad]
  double* sums;
  unsigned long long* counts;
  double* cost;
  int* labels;
  long long n;
  int d, k, kpad;
  int wd8;   // slots of a workspace row (wd / 8)
  int mode;  // 0 labels/cost only, 1 combine in LDS, 2 straight to global
  int lps;   // log2 of the lanes that share a point in the accumulation
  int vec;   // d % 8 == 0 and X 16-byte aligned: stage with 16-byte loads
};

__host__ __device__ constexpr int kb_tile_bytes(int ks, int pt, int ns, int t) {
  return 16 * (4 * ks + 1) * (t * 16 * ns + 64 * pt) + 4 * 16 * ns + 12 * 64 * pt;
}

__device__ __forceinline__ float kb_widen(unsigned bits) { return __uint_as_float(bits << 16); }

__device__ __forceinline__ unsigned kb_rne(float f) {  // fp32 -> bf16 bits, round to nearest even
  const unsigned u = __float_as_uint(f);
  if ((u & 0x7fffffffu) > 0x7f800000u) return (u >> 16) | 0x40u;
  return (u + 0x7fffu + ((u >> 16) & 1u)) >> 16;
}

// One wave per workspace row j < kpad: the T piece planes (zero past k and
// past d) and cn[j], +inf past k.
template <int T>
__global__ __launch_bounds__(KB_THREADS) void kmeans_bf16_split_kernel(const float* __restrict__ C,
                                                                       uint16_t* __restrict__ P,
                                                                       float* __restrict__ cn, int d, int k, int kpad,
                                                                       int wd) {
  __shared__ float row[4][KB_MAXD];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int j = blockIdx.x * 4 + wave;  // the grid is kpad / 4 workgroups
  for (int c = lane; c < wd; c += 64) {
    float r = (j < k && c < d) ? C[(size_t)j * d + c] : 0.f;
    float ct = 0.f;
#pragma unroll
    for (int t = 0; t < T; ++t) {
      const unsigned h = kb_rne(r);
      const float f = kb_widen(h);
      P[((size_t)t * kpad + j) * wd + c] = (uint16_t)h;
      r -= f;   // exact
      ct += f;  // exact: at most 24 significant bits for T <= 3
    }
    if (c < d) row[wave][c] = ct;
  }
  __syncthreads();
  if (lane == 0) {
    float s = 0.f;
    for (int c = 0; c < d; ++c) s = fmaf(row[wave][c], row[wave][c], s);
    cn[j] = j < k ? s : INFINITY;
  }
}

// Stage points [row0, row0 + ROWS) into LDS rows of 4 KS slots (stride 4 KS + 1),
// zero past either edge; every load is from a clamped, always valid address.
template <int KS, int ROWS>
__device__ __forceinline__ void kb_stage_x(u32x4* __restrict__ dst, const uint16_t* __restrict__ X, long long row0,
                                           long long n, int d, int vec, int tid) {
  constexpr int W8 = 4 * KS, W = 32 * KS, S = 4 * KS + 1;
  if (vec) {
#pragma unroll 2
    for (int e = tid; e < ROWS * W8; e += KB_THREADS) {
      const int r = e / W8, c = e % W8;
      const bool ok = row0 + r < n && 8 * c < d;
      u32x4 v = *reinterpret_cast<const u32x4*>(X + (ok ? (size_t)(row0 + r) * d + 8 * c : (size_t)0));
      if (!ok) v = u32x4{0u, 0u, 0u, 0u};
      dst[r * S + c] = v;
    }
  } else {
    uint16_t* d16 = reinterpret_cast<uint16_t*>(dst);
#pragma unroll 8
    for (int e = tid; e < ROWS * W; e += KB_THREADS) {
      const int r = e / W, c = e % W;
      const bool ok = row0 + r < n && c < d;
      const uint16_t v = X[ok ? (size_t)(row0 + r) * d + c : (size_t)0];
      d16[r * S * 8 + c] = ok ? v : (uint16_t)0;
    }
  }
}

template <int KS, int PT, int NS, int T>
__global__ __launch_bounds__(KB_THREADS) __attribute__((amdgpu_waves_per_eu(KS <= 4 ? 2 : 1))) void kmeans_bf16_step_kernel(const KbArgs p) {
  constexpr int S = 4 * KS + 1;  // row stride in slots
  constexpr int W8 = 4 * KS;     // slots of a row
  constexpr int PW = 64 * PT;    // points per super-tile
  constexpr int CT = 16 * NS;    // centroids per LDS tile
  extern __shared__ u32x4 kb_lds[];
  u32x4* Cs = kb_lds;                       // [T][CT][S] piece planes of the centroid tile
  u32x4* Xs = Cs + T * CT * S;              // [PW][S]    point super-tile
  float* cnS = (float*)(Xs + PW * S);       // [CT]  |C_T|^2, +inf on padding
  float* xnS = cnS + CT;                    // [PW]  |x|^2
  float* bestS = xnS + PW;                  // [PW]  winning score
  int* labS = (int*)(bestS + PW);           // [PW]  winning index
  float* ls = (float*)(labS + PW);          // [k][d] mode 1: fp32 partial sums
  unsigned* lc = (unsigned*)(ls + (size_t)p.k * p.d);  // [k] mode 1: counts
  const uint16_t* X16 = reinterpret_cast<const uint16_t*>(Xs);

  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int col = lane & 15, g = lane >> 4;
  const int d = p.d, k = p.k;
  const long long n = p.n;
  const int nct = (k + CT - 1) / CT;
  const long long nsuper = (n + PW - 1) / PW;

  if (p.mode == 1) {
    for (int e = tid; e < k * d; e += KB_THREADS) ls[e] = 0.f;
    for (int e = tid; e < k; e += KB_THREADS) lc[e] = 0u;
  }

  double mycost = 0.0;
  bool cstaged = false;
  for (long long st = blockIdx.x; st < nsuper; st += gridDim.x) {
    const long long base = st * PW;
    bf16x8 a[PT][KS];
    float best[PT][4], xn[PT];
    int bidx[PT][4];
#pragma unroll
    for (int t = 0; t < PT; ++t)
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        best[t][i] = INFINITY;
        bidx[t][i] = 0;
      }

    for (int ct = 0; ct < nct; ++ct) {
      const bool stage_c = nct > 1 || !cstaged;
      __syncthreads();  // every reader of Cs / cnS / Xs / labS of the step before is done
      if (stage_c) {
#pragma unroll 2
        for (int e = tid; e < T * CT * W8; e += KB_THREADS) {
          const int t = e / (CT * W8), r = (e / W8) % CT, c = e % W8;
          const bool ok = c < p.wd8;
          u32x4 v = p.P[((size_t)t * p.kpad + ct * CT + r) * p.wd8 + (ok ? c : 0)];
          if (!ok) v = u32x4{0u, 0u, 0u, 0u};
          Cs[(t * CT + r) * S + c] = v;
        }
        if (tid < CT) cnS[tid] = p.cn[ct * CT + tid];
        cstaged = true;
      }
      if (ct == 0) kb_stage_x<KS, PW>(Xs, p.X, base, n, d, p.vec, tid);
      __syncthreads();
      if (ct == 0) {  // A fragments into registers, and |x|^2
#pragma unroll
        for (int t = 0; t < PT; ++t) {
          const u32x4* xr = Xs + (wave * (16 * PT) + t * 16 + col) * S + g;
          float s = 0.f;
#pragma unroll
          for (int ks = 0; ks < KS; ++ks) {
            const u32x4 v = xr[4 * ks];
            a[t][ks] = __builtin_bit_cast(bf16x8, v);
#pragma unroll
            for (int w = 0; w < 4; ++w) {
              const float lo = kb_widen(v[w] & 0xffffu), hi = __uint_as_float(v[w] & 0xffff0000u);
              s = fmaf(lo, lo, s);
              s = fmaf(hi, hi, s);
            }
          }
          s += __shfl_xor(s, 16);
          s += __shfl_xor(s, 32);
          xn[t] = s;
        }
      }

      // two column tiles at a time (the loop is kept rolled: it bounds the live
      // B fragments and accumulators so two waves fit a SIMD)
      constexpr int NG = NS >= 2 ? 2 : 1;
#pragma unroll 1
      for (int s0 = 0; s0 < NS; s0 += NG) {
        f32x4 acc[NG][PT];
#pragma unroll
        for (int s = 0; s < NG; ++s)
#pragma unroll
          for (int t = 0; t < PT; ++t) acc[s][t] = f32x4{0.f, 0.f, 0.f, 0.f};
        const u32x4* Cb = Cs + (s0 * 16 + col) * S + g;
#pragma unroll
        for (int ks = 0; ks < KS; ++ks)
#pragma unroll
          for (int pc = 0; pc < T; ++pc)
#pragma unroll
            for (int s = 0; s < NG; ++s) {
              const bf16x8 b = __builtin_bit_cast(bf16x8, Cb[(pc * CT + s * 16) * S + 4 * ks]);
#pragma unroll
              for (int t = 0; t < PT; ++t)
                acc[s][t] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a[t][ks], b, acc[s][t], 0, 0, 0);
            }
        // C/D layout: col = lane & 15, row = 4 (lane >> 4) + reg.  Indices reach a
        // lane in ascending order and the compare is strict: the lowest wins.
#pragma unroll
        for (int s = 0; s < NG; ++s) {
          const float cn = cnS[(s0 + s) * 16 + col];
          const int j = ct * CT + (s0 + s) * 16 + col;
#pragma unroll
          for (int t = 0; t < PT; ++t)
#pragma unroll
            for (int i = 0; i < 4; ++i) {
              const float sc = fmaf(-2.f, acc[s][t][i], cn);
              if (sc < best[t][i]) {
                best[t][i] = sc;
                bidx[t][i] = j;
              }
            }
        }
      }
    }

    // the 16 lanes that share rows: (score, index) lexicographic minimum
#pragma unroll
    for (int t = 0; t < PT; ++t)
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
          const int q = wave * (16 * PT) + t * 16 + g * 4 + i;
          j = min(max(j, 0), k - 1);
          labS[q] = j;
          bestS[q] = s;
          if (p.labels && base + q < n) p.labels[base + q] = j;
        }
      }
    if (g == 0) {
#pragma unroll
      for (int t = 0; t < PT; ++t) xnS[wave * (16 * PT) + t * 16 + col] = xn[t];
    }
    __syncthreads();

    if (tid < PW && base + tid < n) mycost += (double)fmaxf(0.f, xnS[tid] + bestS[tid]);

    if (p.mode != 0) {  // add the rows into their clusters: 2^lps lanes per point, along d
      const int lp = 1 << p.lps, ppi = 64 >> p.lps;
      const int cl = lane & (lp - 1);
      for (int q = wave * ppi + (lane >> p.lps); q < PW; q += 4 * ppi) {
        const long long i = base + q;
        if (i >= n) continue;
        const int L = labS[q];
        const uint16_t* xr = X16 + q * S * 8;
        if (p.mode == 1) {
          for (int c = cl; c < d; c += lp) atomicAdd(&ls[L * d + c], kb_widen(xr[c]));
          if (cl == 0) atomicAdd(&lc[L], 1u);
        } else {
          if (p.sums)
            for (int c = cl; c < d; c += lp) unsafeAtomicAdd(&p.sums[(size_t)L * d + c], (double)kb_widen(xr[c]));
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
      for (int e = tid; e < k * d; e += KB_THREADS)
        if (lc[e / d]) unsafeAtomicAdd(&p.sums[e], (double)ls[e]);
    if (p.counts)
      for (int j = tid; j < k; j += KB_THREADS)
        if (lc[j]) atomicAdd(&p.counts[j], (unsigned long long)lc[j]);
  }
}

// the variant that serves d: k-steps, point tiles per wave, column tiles
struct KbVariant {
  int ks, pt, ns;
};
inline KbVariant kb_variant(int d) {
  if (d <= 32) return {1, 4, 4};
  if (d <= 64) return {2, 4, 4};
  if (d <= 128) return {4, 2, 2};
  if (d <= 256) return {8, 2, 2};
  return {16, 1, 1};
}

struct KbDevice {
  int lds = 0;  // LDS a workgroup may take (bytes)
  int cus = 0;
};

inline const KbDevice* kb_device() {
  static KbDevice devs[64];
  int dev = 0;
  if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= 64) return nullptr;
  KbDevice& D = devs[dev];
  if (D.cus == 0) {
    int lds = 0, cus = 0;
    if (hipDeviceGetAttribute(&lds, hipDeviceAttributeMaxSharedMemoryPerBlock, dev) != hipSuccess ||
        hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess || cus <= 0)
      return nullptr;
    D.lds = lds < KB_LDS_MAX ? lds : KB_LDS_MAX;
    D.cus = cus;
  }
  return &D;
}

// largest k whose [k, d] fp32 partial sums and k counts fit beside the tiles
// (those of T = 3, whatever T a step runs: one limit per d)
inline int kb_lds_limit(int d, int lds) {
  const KbVariant v = kb_variant(d);
  const long long left = (long long)lds - kb_tile_bytes(v.ks, v.pt, v.ns, 3);
  return left <= 0 ? 0 : (int)(left / (4ll * (d + 1)));
}

template <int KS, int PT, int NS, int T>
int kb_launch(const KbArgs& a, size_t lds, unsigned grid, hipStream_t s) {
  static bool lds_attr = false;  // dynamic LDS above 64 KiB must be allowed once
  if (!lds_attr) {
    (void)hipFuncSetAttribute((const void*)kmeans_bf16_step_kernel<KS, PT, NS, T>,
                              hipFuncAttributeMaxDynamicSharedMemorySize, KB_LDS_MAX);
    lds_attr = true;
  }
  hipLaunchKernelGGL((kmeans_bf16_step_kernel<KS, PT, NS, T>), dim3(grid), dim3(KB_THREADS), lds, s, a);
  return (int)hipGetLastError();
}

template <int T>
int kb_step(const KbArgs& a, const KbVariant& v, size_t lds, unsigned grid, const float* C, uint16_t* P, float* cn,
            hipStream_t s) {
  hipLaunchKernelGGL((kmeans_bf16_split_kernel<T>), dim3(a.kpad / 4), dim3(KB_THREADS), 0, s, C, P, cn, a.d, a.k,
                     a.kpad, 8 * a.wd8);
  const int rc = (int)hipGetLastError();
  if (rc != 0 || a.n == 0) return rc;
  switch (v.ks) {
    case 1: return kb_launch<1, 4, 4, T>(a, lds, grid, s);
    case 2: return kb_launch<2, 4, 4, T>(a, lds, grid, s);
    case 4: return kb_launch<4, 2, 2, T>(a, lds, grid, s);
    case 8: return kb_launch<8, 2, 2, T>(a, lds, grid, s);
    default: return kb_launch<16, 1, 1, T>(a, lds, grid, s);
  }
}

inline bool kb_shape_ok(int d, int k, int terms) {
  return d >= 1 && d <= KB_MAXD && k >= 1 && k <= KB_MAXK && terms >= 1 && terms <= 3;
}
inline int kb_kpad(int k) { return (k + KB_KPAD - 1) / KB_KPAD * KB_KPAD; }
inline int kb_wd(int d) { return (d + 31) / 32 * 32; }

}  // namespace

extern "C" {

// Bytes of the workspace of a step: bf16 planes [terms][kpad][wd], then fp32
// cn [kpad]; kpad = k rounded up to 64, wd = d rounded up to 32.
int mr_kmeans_bf16_workspace_bytes(int d, int k, int terms) {
  if (!kb_shape_ok(d, k, terms)) return -2;
  return 2 * terms * kb_kpad(k) * kb_wd(d) + 4 * kb_kpad(k);
}

// Largest k for which a bf16 step at this d combines its sums in LDS (mode 1).
int mr_kmeans_bf16_lds_limit(int d) {
  if (d < 1 || d > KB_MAXD) return -2;
  const KbDevice* D = kb_device();
  return D ? kb_lds_limit(d, D->lds) : -1;
}

// One bf16 k-means map step (see the header): the prologue fills `workspace`
// (16-byte aligned, mr_kmeans_bf16_workspace_bytes) from C, then the points
// are assigned against it.  n == 0 runs the prologue alone.  sums / counts /
// cost are added into and may each be null; labels may be null.  -2: shape or
// terms out of range, or a misaligned workspace;  -3: the LDS cannot hold the tiles.
int mr_kmeans_bf16_step(const void* X, const void* C, long long n, int d, int k, int terms, void* workspace,
                        void* sums, void* counts, void* cost, void* labels, hipStream_t s) {
  if (!kb_shape_ok(d, k, terms) || n < 0 || !workspace || ((uintptr_t)workspace & 15)) return -2;
  const KbDevice* D = kb_device();
  if (!D) return -1;
  const KbVariant v = kb_variant(d);
  size_t lds = (size_t)kb_tile_bytes(v.ks, v.pt, v.ns, terms);
  if (lds > (size_t)D->lds) return -3;
  KbArgs a;
  a.kpad = kb_kpad(k);
  a.wd8 = kb_wd(d) / 8;
  uint16_t* P = (uint16_t*)workspace;
  float* cn = (float*)(P + (size_t)terms * a.kpad * kb_wd(d));
  a.X = (const uint16_t*)X;
  a.P = (const u32x4*)P;
  a.cn = cn;
  a.sums = (double*)sums;
  a.counts = (unsigned long long*)counts;
  a.cost = (double*)cost;
  a.labels = (int*)labels;
  a.n = n;
  a.d = d;
  a.k = k;
  a.mode = (!sums && !counts) ? 0 : (k <= kb_lds_limit(d, D->lds) ? 1 : 2);
  if (a.mode == 1) lds += 4 * (size_t)k * (d + 1);
  a.lps = 0;
  while (a.lps < 6 && (1 << a.lps) < d) ++a.lps;
  a.vec = (d % 8 == 0 && ((uintptr_t)X & 15) == 0) ? 1 : 0;
  const long long pw = 64 * v.pt, nsuper = (n + pw - 1) / pw;
  // resident workgroups per CU: by LDS, and at most 2 (the registers allow two waves per SIMD)
  long long wpc = KB_LDS_MAX / (long long)lds;
  wpc = wpc < 1 ? 1 : wpc > 2 ? 2 : wpc;
  const unsigned grid = (unsigned)(nsuper < wpc * D->cus ? nsuper : wpc * D->cus);
  if (terms == 1) return kb_step<1>(a, v, lds, grid, (const float*)C, P, cn, s);
  if (terms == 2) return kb_step<2>(a, v, lds, grid, (const float*)C, P, cn, s);
  return kb_step<3>(a, v, lds, grid, (const float*)C, P, cn, s);
}

}  // extern "C"
