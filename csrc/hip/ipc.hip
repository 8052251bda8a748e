// ipc.hip — device-resident intermediate files shared between worker
// processes (the "hbm" storage of runtime/hbm_store.py).
//
// The reference's storages all work across worker processes and hosts:
// GridFS through mongod, "shared" through NFS, "sshfs" through scp
// (/root/reference/mapreduce/fs.lua:185-208); a reduce job reads the map files
// any worker wrote (job.lua:253-260).  On one MI355X node the natural store is
// HBM itself: a map worker keeps its partition files in an arena of device
// memory it exports with hipIpcGetMemHandle; the coordinator's file entry holds
// the handle and the file's place in the arena; a reducer on any GPU of the
// node maps the arena (hipIpcOpenMemHandle) and pulls the files it needs with
// ONE gather-copy launch over xGMI (or inside the GPU) into its own buffer, where
// ONE decode launch turns the columnar files (runtime/codec.py MRC1, MRC2 for
// the general plane's typed folds, MRL1 for its value lists) into the reduce
// table's input columns.  The
// write side of a device map on a GPU worker is its mirror.  A fold map (word
// count and the other fold ops of runtime/job.py::_run_device_map_locked): ONE
// plan launch sizes the partition files from the sorted tail's columns, ONE
// encode launch writes them as MRC1 files straight into the arena.  A typed-fold
// map (runtime/job.py::_run_generic_map, a column spec such as
// ("f64:mean", "f64:max", "count")): the same plan launch over the sorted
// columns of parallel/generic.py::order_fold, ONE encode launch that writes the
// MRC2 files.  A list map (the same job without device_reduce or with a concat
// op, scalar i64 / f64 values): ONE plan launch over order_lists' partition
// counts, key offsets and list offsets, ONE encode launch that writes the MRL1
// files (every key with its value list); its reducer decodes the pulled files
// with ONE launch into rows and (value, row) pairs that the list-mode table
// merges per key.  For those jobs no byte of the intermediate data goes through
// host memory or the coordinator's socket: only the plan (partition row and
// key-byte counts, the tail's flags: 8 * (2 * nparts + 4) bytes; a list map's
// rows, key bytes and values: 8 * (3 * nparts + 3) bytes) comes to the host.
// List maps with tuple or byte-string values (MRK1 records), host maps, a fold
// map whose tail raised a flag and a typed fold or list map past the plan's
// limits are still encoded on the host and uploaded (HBMStore.put_many); the
// reduce side of the columnar ones stays on the device all the same.
//
//   mr_ipc_alloc / mr_ipc_free        hipMalloc'd arena chunks (exportable)
//   mr_ipc_handle                     the 64-byte hipIpcMemHandle_t of a chunk
//   mr_ipc_open / mr_ipc_close        a peer's chunk in this process
//   mr_gather_copy                    n (src, dst, len) copies in one launch
//   mr_mrc1_decode                    MRC1 files in one buffer -> hi, lo, val, rep
//   mr_mrc1_plan                      partition counts + sorted offsets -> rows and key bytes per file
//   mr_mrc1_encode                    sorted columns + key bytes -> every MRC1 file of a map job
//   mr_mrc2_decode                    MRC2 files in one buffer -> hi, lo, rep, k typed value columns
//   mr_mrc2_encode                    sorted columns + key bytes -> every MRC2 file of a map job
//   mr_mrl1_plan                      partition counts + key and list offsets -> rows, key bytes, values per file
//   mr_mrl1_encode                    sorted keys + value lists + key bytes -> every MRL1 file of a map job
//   mr_mrl1_decode                    MRL1 files in one buffer -> hi, lo, rep per row; bits, row per value
#include <hip/hip_runtime.h>
#include <cstring>
#include "mr_common.h"

namespace mr {

// One workgroup per copy run of up to GC_CHUNK bytes: 16-byte vector loads and
// stores when source, destination and length allow, else bytes.  Sources may be
// peer memory (an IPC-mapped chunk of another GPU: the loads cross xGMI).
constexpr int GC_T = 256;
constexpr u64 GC_CHUNK = 1ull << 18;

__global__ void __launch_bounds__(GC_T) gather_copy_kernel(const u64* __restrict__ srcs, const u64* __restrict__ dsts,
                                                           const u64* __restrict__ lens,
                                                           const u64* __restrict__ chunk_start, u32 n) {
  // chunk_start[i] = first chunk of copy i (prefix over ceil(len / GC_CHUNK))
  const u64 c = blockIdx.x;
  u32 lo = 0, hi = n;
  while (hi - lo > 1) {
    const u32 mid = (lo + hi) / 2;
    if (chunk_start[mid] <= c) lo = mid; else hi = mid;
  }
  const u32 i = lo;
  const u64 off = (c - chunk_start[i]) * GC_CHUNK;
  const u64 len = lens[i];
  if (off >= len) return;
  const u64 m = len - off < GC_CHUNK ? len - off : GC_CHUNK;
  const u8* s = reinterpret_cast<const u8*>(srcs[i]) + off;
  u8* d = reinterpret_cast<u8*>(dsts[i]) + off;
  if ((((uintptr_t)s ^ (uintptr_t)d) & 15) == 0) {
    // same offset mod 16 on both sides: a byte head up to the next 16-byte
    // boundary, then 16-byte vectors, then a byte tail
    u64 head = (16 - ((uintptr_t)s & 15)) & 15;
    if (head > m) head = m;
    if (threadIdx.x < head) d[threadIdx.x] = s[threadIdx.x];
    const u64 n16 = (m - head) / 16;
    const uint4* s4 = reinterpret_cast<const uint4*>(s + head);
    uint4* d4 = reinterpret_cast<uint4*>(d + head);
    for (u64 k = threadIdx.x; k < n16; k += GC_T) d4[k] = s4[k];
    for (u64 k = head + n16 * 16 + threadIdx.x; k < m; k += GC_T) d[k] = s[k];
  } else {
    for (u64 k = threadIdx.x; k < m; k += GC_T) d[k] = s[k];
  }
}

// MRC1 file j at byte base[j] of buf (base[j] % 8 == 4, so its 8-byte columns
// after the 20-byte header are aligned): rows rstart[j] .. rstart[j+1] of the
// output.  Layout (codec.encode_columnar): "MRC1" n nb | hi[n] lo[n] val[n]
// key_off[n+1] | key bytes.  rep = (byte offset of the key in buf) << 24 | len,
// so buf itself is the key-byte source of the reduce table.
constexpr int DC_T = 256;
__global__ void __launch_bounds__(DC_T) mrc1_decode_kernel(const u8* __restrict__ buf, const u64* __restrict__ base,
                                                           const u64* __restrict__ rstart, u32 nfiles, u64 nrows,
                                                           u64* __restrict__ o_hi, u64* __restrict__ o_lo,
                                                           long long* __restrict__ o_val, u64* __restrict__ o_rep) {
  const u64 r = (u64)blockIdx.x * DC_T + threadIdx.x;
  if (r >= nrows) return;
  u32 lo = 0, hi = nfiles;
  while (hi - lo > 1) {
    const u32 mid = (lo + hi) / 2;
    if (rstart[mid] <= r) lo = mid; else hi = mid;
  }
  const u64 n = rstart[lo + 1] - rstart[lo];
  const u64 k = r - rstart[lo];
  const u64 b = base[lo] + 20;
  const u64* col = reinterpret_cast<const u64*>(buf + b);
  const long long* koff = reinterpret_cast<const long long*>(col + 3 * n);
  const u64 kb = b + 8 * (4 * n + 1);
  const long long o = koff[k];
  o_hi[r] = col[k];
  o_lo[r] = col[n + k];
  o_val[r] = (long long)col[2 * n + k];
  o_rep[r] = make_rep(kb + (u64)o, (u64)(koff[k + 1] - o));
}

// Rows and key bytes of every partition's file, and what the host needs to
// decide whether the device may write them: out = i64 [2 * nparts + 4]:
// rows[nparts] | key bytes[nparts] | bad | err | off[n] | sum of the counts.
// bounds = the exclusive scan of the counts (clamped to n: counts of a sort that
// gave up index nothing outside off's n + 1 entries).  One block; thread p sums
// the p counts before its own from LDS (at most 255 broadcast reads: the
// quadratic scan is deliberate, nparts <= 256 and a shuffle scan saves nothing
// a launch of this size would show).
constexpr int PL_T = 256;
__global__ void __launch_bounds__(PL_T) mrc1_plan_kernel(const long long* __restrict__ counts,
                                                         const long long* __restrict__ off, u64 n, u32 nparts,
                                                         const u32* __restrict__ bad, const u32* __restrict__ err,
                                                         long long* __restrict__ out) {
  __shared__ u64 cnt[PL_T];
  const u32 t = threadIdx.x;
  cnt[t] = t < nparts ? (u64)counts[t] : 0;
  __syncthreads();
  u64 b0 = 0;
  for (u32 q = 0; q < t; ++q) b0 += cnt[q];
  u64 b1 = b0 + cnt[t];
  if (t < nparts) {
    const u64 a = b0 < n ? b0 : n, b = b1 < n ? b1 : n;
    out[t] = (long long)cnt[t];
    out[nparts + t] = off[b] - off[a];
  }
  if (t == PL_T - 1) {
    out[2 * nparts] = (long long)bad[0];
    out[2 * nparts + 1] = (long long)err[0];
    out[2 * nparts + 2] = off[n];
    out[2 * nparts + 3] = (long long)b1;
  }
}

// One workgroup per EN_UNIT bytes of one file.  A file of n rows at dst
// (dst % 16 == 4) is walked as the byte stream t = file offset + 4, so that
// t % 16 == 0 is a 16-byte boundary of the destination: unit k of the file owns
// t in [k * EN_UNIT, (k + 1) * EN_UNIT), a file of F bytes has
// ceil((F + 4) / EN_UNIT) units (mr_mrc1_encode_units).  In stream terms:
//   t = 4             "MRC1"
//   t = 8 + 8 w       word w: n | nb | hi[n] | lo[n] | val[n] | key_off[n + 1]
//   t = 32 + 32 n     key bytes (a 16-byte boundary)
// Words go out as 8-byte stores.  Key bytes go out as 16-byte stores, every
// unit's first one on a 16-byte boundary; their source blob + off[a] has any
// alignment: each 16-byte piece is cut out of the two aligned 16-byte vectors
// round it (the shift is the same for the whole unit), bytes only for the
// file's last < 16 bytes and for a piece whose vectors would reach outside
// [blob, blob + blob_cap).
constexpr int EN_T = 256;
constexpr u64 EN_UNIT = 1ull << 14;

__device__ __forceinline__ uint4 cut16(uint4 lo, uint4 hi, u32 sh) {
  // bytes sh .. sh + 15 of the 32 bytes lo | hi (0 < sh < 16)
  const u64 x0 = (u64)lo.x | ((u64)lo.y << 32), x1 = (u64)lo.z | ((u64)lo.w << 32);
  const u64 x2 = (u64)hi.x | ((u64)hi.y << 32), x3 = (u64)hi.z | ((u64)hi.w << 32);
  const bool up = sh >= 8;
  const u64 y0 = up ? x1 : x0, y1 = up ? x2 : x1, y2 = up ? x3 : x2;
  const u32 r = (sh & 7) * 8;
  const u64 o0 = r ? (y0 >> r) | (y1 << (64 - r)) : y0;
  const u64 o1 = r ? (y1 >> r) | (y2 << (64 - r)) : y1;
  return make_uint4((u32)o0, (u32)(o0 >> 32), (u32)o1, (u32)(o1 >> 32));
}

// len key bytes from blob + so to d (d % 16 == 0): 16-byte stores cut out of the
// aligned source vectors, bytes for the last < 16 and for a piece whose vectors
// would reach outside [blob, blob + blob_cap).  One workgroup, thread t of EN_T.
__device__ __forceinline__ void put_key_bytes(u8* __restrict__ d, const u8* __restrict__ blob, u64 blob_cap, u64 so,
                                              u64 len, u32 t) {
  const uintptr_t sa = (uintptr_t)blob + so;
  const u32 sh = (u32)(sa & 15);
  const u64 n16 = len / 16;
  const uintptr_t blo = (uintptr_t)blob, bhi = (uintptr_t)blob + blob_cap;
  for (u64 k = t; k < n16; k += EN_T) {
    const uintptr_t va = sa - sh + 16 * k;  // the aligned vector that holds the piece's first byte
    uint4 o;
    if (va >= blo && va + (sh ? 32 : 16) <= bhi) {
      const uint4 x = *reinterpret_cast<const uint4*>(va);
      o = sh ? cut16(x, *reinterpret_cast<const uint4*>(va + 16), sh) : x;
    } else {
      u32 w[4] = {0, 0, 0, 0};
#pragma unroll
      for (int i = 0; i < 16; ++i) {
        const u64 p = so + 16 * k + i;
        const u32 byte = p < blob_cap ? blob[p] : 0u;
        w[i >> 2] |= byte << (8 * (i & 3));
      }
      o = make_uint4(w[0], w[1], w[2], w[3]);
    }
    reinterpret_cast<uint4*>(d)[k] = o;
  }
  const u64 done = 16 * n16;
  const u64 rem = len - done;  // < 16: the file's last bytes
  if (t < rem) {
    const u64 p = so + done + t;
    d[done + t] = p < blob_cap ? blob[p] : (u8)0;
  }
}

__global__ void __launch_bounds__(EN_T) mrc1_encode_kernel(const u64* __restrict__ hi, const u64* __restrict__ lo,
                                                           const u64* __restrict__ val,
                                                           const long long* __restrict__ off,
                                                           const u8* __restrict__ blob, u64 blob_cap,
                                                           const u64* __restrict__ dsts, const u64* __restrict__ rstart,
                                                           const u64* __restrict__ rows,
                                                           const u64* __restrict__ unit_start, u32 nfiles) {
  const u64 c = blockIdx.x;
  u32 flo = 0, fhi = nfiles;
  while (fhi - flo > 1) {
    const u32 mid = (flo + fhi) / 2;
    if (unit_start[mid] <= c) flo = mid; else fhi = mid;
  }
  const u32 j = flo;
  const u64 n = rows[j], a = rstart[j];
  const u64 o0 = (u64)off[a];
  const u64 nb = (u64)off[a + n] - o0;
  const u64 tw = 32 + 32 * n;   // stream position of the key bytes
  const u64 tend = tw + nb;     // ... and of the file's end
  const u64 t0 = (c - unit_start[j]) * EN_UNIT;
  if (t0 >= tend) return;
  const u64 t1 = t0 + EN_UNIT < tend ? t0 + EN_UNIT : tend;
  u8* base = reinterpret_cast<u8*>(dsts[j]) - 4;  // stream position 0: a 16-byte boundary
  const u32 t = threadIdx.x;
  if (t0 == 0 && t == 0) *reinterpret_cast<u32*>(base + 4) = 0x3143524Du;  // "MRC1"
  if (t0 < tw) {
    const u64 w0 = t0 ? (t0 - 8) / 8 : 0;
    const u64 w1 = ((t1 < tw ? t1 : tw) - 8) / 8;
    u64* dw = reinterpret_cast<u64*>(base + 8);
    for (u64 w = w0 + t; w < w1; w += EN_T) {
      u64 v;
      if (w < 2) v = w ? nb : n;
      else if (w < 2 + n) v = hi[a + (w - 2)];
      else if (w < 2 + 2 * n) v = lo[a + (w - 2 - n)];
      else if (w < 2 + 3 * n) v = val[a + (w - 2 - 2 * n)];
      else v = (u64)off[a + (w - 2 - 3 * n)] - o0;
      dw[w] = v;
    }
  }
  if (t1 > tw) {
    const u64 b0 = (t0 > tw ? t0 : tw) - tw, b1 = t1 - tw;  // key bytes [b0, b1) of the file; b0 % 16 == 0
    put_key_bytes(base + tw + b0, blob, blob_cap, o0 + b0, b1 - b0, t);
  }
}

// MRC2 (codec.encode_columns): the typed folds' files.  k <= MRC2_MAXK value
// columns of dtype code 0 = i64, 1 = f64 (8 bytes a value), 2 = f32 (4 bytes);
// with k <= 8 the header is 36 bytes: "MRC2" n nb k | 8 code bytes.  A file at
// 4 mod 8 has its hi, lo and key_off words aligned; a value column behind an
// f32 column of odd n lies at 4 mod 8, and so may the key bytes.
constexpr int MRC2_MAXK = 8;
struct Mrc2Cols {
  void* col[MRC2_MAXK];  // encode: the sorted source columns; decode: the output columns
  u32 code[MRC2_MAXK];
  u32 k;
};

__device__ __forceinline__ u32 mrc2_width(u32 code) { return code == 2 ? 4u : 8u; }

// The 4-byte word at byte p (p % 4 == 0) of a file's value region (its k
// columns of n values back to back), read from rows a .. a + n of the source
// columns
__device__ __forceinline__ u32 mrc2_value_word(const Mrc2Cols& cs, u64 n, u64 a, u64 p) {
  u32 v = 0;
  bool found = false;
#pragma unroll
  for (int c = 0; c < MRC2_MAXK; ++c) {
    if ((u32)c < cs.k && !found) {
      const u32 w = mrc2_width(cs.code[c]);
      const u64 sz = n * w;
      if (p < sz) {
        v = *reinterpret_cast<const u32*>(static_cast<const u8*>(cs.col[c]) + a * w + p);
        found = true;
      } else {
        p -= sz;
      }
    }
  }
  return v;
}

// MRC2 files at base[j] of buf (base[j] % 8 == 4) -> hi, lo, rep and the k
// typed value columns of rows rstart[j] .. rstart[j + 1]; every file has the
// same k and codes (cs).  rep indexes buf, as in mrc1_decode_kernel.  A value
// column at 4 mod 8 is read in 4-byte halves.
__global__ void __launch_bounds__(DC_T) mrc2_decode_kernel(const u8* __restrict__ buf, const u64* __restrict__ base,
                                                           const u64* __restrict__ rstart, u32 nfiles, u64 nrows,
                                                           u64* __restrict__ o_hi, u64* __restrict__ o_lo,
                                                           u64* __restrict__ o_rep, const Mrc2Cols cs) {
  const u64 r = (u64)blockIdx.x * DC_T + threadIdx.x;
  if (r >= nrows) return;
  u32 lo = 0, hi = nfiles;
  while (hi - lo > 1) {
    const u32 mid = (lo + hi) / 2;
    if (rstart[mid] <= r) lo = mid; else hi = mid;
  }
  const u64 n = rstart[lo + 1] - rstart[lo];
  const u64 i = r - rstart[lo];
  const u64 b = base[lo] + 36;
  const u64* col = reinterpret_cast<const u64*>(buf + b);
  const long long* koff = reinterpret_cast<const long long*>(col + 2 * n);
  const long long o = koff[i];
  o_hi[r] = col[i];
  o_lo[r] = col[n + i];
  u64 vb = b + 8 * (3 * n + 1);  // the value columns, then the key bytes
#pragma unroll
  for (int c = 0; c < MRC2_MAXK; ++c) {
    if ((u32)c < cs.k) {
      if (mrc2_width(cs.code[c]) == 4) {
        static_cast<u32*>(cs.col[c])[r] = *reinterpret_cast<const u32*>(buf + vb + 4 * i);
        vb += 4 * n;
      } else {
        const u8* s = buf + vb + 8 * i;
        u64 v;
        if (vb & 7) {
          const u32* h = reinterpret_cast<const u32*>(s);
          v = (u64)h[0] | ((u64)h[1] << 32);
        } else {
          v = *reinterpret_cast<const u64*>(s);
        }
        static_cast<u64*>(cs.col[c])[r] = v;
        vb += 8 * n;
      }
    }
  }
  o_rep[r] = make_rep(vb + (u64)o, (u64)(koff[i + 1] - o));
}

// One workgroup per EN_UNIT bytes of one MRC2 file, walked like an MRC1 file as
// the stream t = file offset + 4 (dst % 16 == 4):
//   t = 4               "MRC2"
//   t = 8 + 8 w         word w: n | nb | k | codes | hi[n] | lo[n] | key_off[n + 1]
//   t = 48 + 24 n       the value region: n * (sum of the widths) bytes, a multiple of 4
//   t = tk              key bytes (tk % 16 is 0, 4, 8 or 12)
// Words go out as 8-byte stores.  The value region goes out in 8-byte slots of
// the stream too, each put together from two 4-byte loads of the columns' 8- or
// 4-byte values (a column behind an odd f32 column is at 4 mod 8 in the file
// and aligned in its source: no wide access is misaligned on either side), a
// last half slot as 4 bytes.  Key bytes: bytes up to the first 16-byte boundary of
// the destination (only behind tk, at most 12), then as in the MRC1 files.
__global__ void __launch_bounds__(EN_T) mrc2_encode_kernel(const u64* __restrict__ hi, const u64* __restrict__ lo,
                                                           const long long* __restrict__ off,
                                                           const u8* __restrict__ blob, u64 blob_cap,
                                                           const u64* __restrict__ dsts, const u64* __restrict__ rstart,
                                                           const u64* __restrict__ rows,
                                                           const u64* __restrict__ unit_start, u32 nfiles,
                                                           const Mrc2Cols cs) {
  const u64 c = blockIdx.x;
  u32 flo = 0, fhi = nfiles;
  while (fhi - flo > 1) {
    const u32 mid = (flo + fhi) / 2;
    if (unit_start[mid] <= c) flo = mid; else fhi = mid;
  }
  const u32 j = flo;
  const u64 n = rows[j], a = rstart[j];
  const u64 o0 = (u64)off[a];
  const u64 nb = (u64)off[a + n] - o0;
  u64 wsum = 0, codes = 0;
#pragma unroll
  for (int q = 0; q < MRC2_MAXK; ++q) {
    if ((u32)q < cs.k) {
      wsum += mrc2_width(cs.code[q]);
      codes |= (u64)(cs.code[q] & 0xFF) << (8 * q);
    }
  }
  const u64 tv = 48 + 24 * n;     // stream position of the value region,
  const u64 tk = tv + n * wsum;   // ... of the key bytes
  const u64 tend = tk + nb;       // ... and of the file's end
  const u64 t0 = (c - unit_start[j]) * EN_UNIT;
  if (t0 >= tend) return;
  const u64 t1 = t0 + EN_UNIT < tend ? t0 + EN_UNIT : tend;
  u8* base = reinterpret_cast<u8*>(dsts[j]) - 4;  // stream position 0: a 16-byte boundary
  const u32 t = threadIdx.x;
  if (t0 == 0 && t == 0) *reinterpret_cast<u32*>(base + 4) = 0x3243524Du;  // "MRC2"
  if (t0 < tv) {
    const u64 w0 = t0 ? (t0 - 8) / 8 : 0;
    const u64 w1 = ((t1 < tv ? t1 : tv) - 8) / 8;
    u64* dw = reinterpret_cast<u64*>(base + 8);
    for (u64 w = w0 + t; w < w1; w += EN_T) {
      u64 v;
      if (w < 4) v = w == 0 ? n : w == 1 ? nb : w == 2 ? (u64)cs.k : codes;
      else if (w < 4 + n) v = hi[a + (w - 4)];
      else if (w < 4 + 2 * n) v = lo[a + (w - 4 - n)];
      else v = (u64)off[a + (w - 4 - 2 * n)] - o0;
      dw[w] = v;
    }
  }
  if (t1 > tv && t0 < tk) {
    // bytes [v0, v1) of the value region: v0 % 8 == 0; v1 % 8 == 4 only at the region's end
    const u64 v0 = (t0 > tv ? t0 : tv) - tv, v1 = (t1 < tk ? t1 : tk) - tv;
    const u64 nslots = (v1 - v0 + 7) / 8;
    u8* d = base + tv;
    for (u64 s = t; s < nslots; s += EN_T) {
      const u64 p = v0 + 8 * s;
      const u32 x0 = mrc2_value_word(cs, n, a, p);
      if (p + 4 < v1) {
        const u32 x1 = mrc2_value_word(cs, n, a, p + 4);
        *reinterpret_cast<u64*>(d + p) = (u64)x0 | ((u64)x1 << 32);
      } else {
        *reinterpret_cast<u32*>(d + p) = x0;
      }
    }
  }
  if (t1 > tk) {
    const u64 b0 = (t0 > tk ? t0 : tk) - tk, b1 = t1 - tk;  // key bytes [b0, b1) of the file
    u8* d = base + tk + b0;
    u64 head = (16 - ((tk + b0) & 15)) & 15;  // != 0 only when b0 == 0: every later unit starts on a boundary
    if (head > b1 - b0) head = b1 - b0;
    if (t < head) {
      const u64 p = o0 + b0 + t;
      d[t] = p < blob_cap ? blob[p] : (u8)0;
    }
    put_key_bytes(d + head, blob, blob_cap, o0 + b0 + head, b1 - b0 - head, t);
  }
}

// MRL1 (codec.encode_lists): the list maps' files: every key with its value
// list (CSR: list_off / list_val, 8-byte words whose bits the kernels only
// move; code 0 = i64, 1 = f64 says how a reader views them).  A file at 4 mod 8
// has every word behind its 36-byte header aligned.
//
// The plan of a list map: out = i64 [3 * nparts + 3]:
// rows[nparts] | key bytes[nparts] | values[nparts] | off[n] | loff[n] | sum of
// the counts.  As in mrc1_plan_kernel the bounds are clamped to n, so counts
// that do not add up index nothing outside the n + 1 entries of off and loff.
__global__ void __launch_bounds__(PL_T) mrl1_plan_kernel(const long long* __restrict__ counts,
                                                         const long long* __restrict__ off,
                                                         const long long* __restrict__ loff, u64 n, u32 nparts,
                                                         long long* __restrict__ out) {
  __shared__ u64 cnt[PL_T];
  const u32 t = threadIdx.x;
  cnt[t] = t < nparts ? (u64)counts[t] : 0;
  __syncthreads();
  u64 b0 = 0;
  for (u32 q = 0; q < t; ++q) b0 += cnt[q];
  u64 b1 = b0 + cnt[t];
  if (t < nparts) {
    const u64 a = b0 < n ? b0 : n, b = b1 < n ? b1 : n;
    out[t] = (long long)cnt[t];
    out[nparts + t] = off[b] - off[a];
    out[2 * nparts + t] = loff[b] - loff[a];
  }
  if (t == PL_T - 1) {
    out[3 * nparts] = off[n];
    out[3 * nparts + 1] = loff[n];
    out[3 * nparts + 2] = (long long)b1;
  }
}

// MRL1 files at base[j] of buf (base[j] % 8 == 4): file j holds rows
// rstart[j] .. rstart[j + 1] and values vstart[j] .. vstart[j + 1] of the
// output.  Thread i decodes row i (hi, lo, rep: rep indexes buf, as in
// mrc1_decode_kernel) and value i (its bits and the global index of its row).
// The value's row is the r of its file with list_off[r] <= k < list_off[r + 1]:
// the LAST r with list_off[r] <= k, so runs of empty lists before it (equal
// offsets) are passed over and those behind it never reached.  The search reads
// list_off where it lies in buf: neighbouring values of a wave walk the same
// upper levels (one address, broadcast) and end in neighbouring words, so the
// loads stay in a few cache lines and nothing is staged in LDS.  Every index is
// bounded by the counts the host checked (job._check_mrl1_layout), whatever
// the offsets in the file say.
__global__ void __launch_bounds__(DC_T) mrl1_decode_kernel(const u8* __restrict__ buf, const u64* __restrict__ base,
                                                           const u64* __restrict__ rstart,
                                                           const u64* __restrict__ vstart, u32 nfiles, u64 nrows,
                                                           u64 nvals, u64* __restrict__ o_hi, u64* __restrict__ o_lo,
                                                           u64* __restrict__ o_rep, u64* __restrict__ o_vbits,
                                                           long long* __restrict__ o_vrow) {
  const u64 i = (u64)blockIdx.x * DC_T + threadIdx.x;
  if (i < nrows) {
    u32 lo = 0, hi = nfiles;
    while (hi - lo > 1) {
      const u32 mid = (lo + hi) / 2;
      if (rstart[mid] <= i) lo = mid; else hi = mid;
    }
    const u64 n = rstart[lo + 1] - rstart[lo];
    const u64 nv = vstart[lo + 1] - vstart[lo];
    const u64 k = i - rstart[lo];
    const u64 b = base[lo] + 36;
    const u64* col = reinterpret_cast<const u64*>(buf + b);
    const long long* koff = reinterpret_cast<const long long*>(col + 2 * n);
    const u64 kb = b + 8 * (4 * n + 2 + nv);  // the key bytes, behind list_off and list_val
    const long long o = koff[k];
    o_hi[i] = col[k];
    o_lo[i] = col[n + k];
    o_rep[i] = make_rep(kb + (u64)o, (u64)(koff[k + 1] - o));
  }
  if (i < nvals) {
    u32 lo = 0, hi = nfiles;
    while (hi - lo > 1) {
      const u32 mid = (lo + hi) / 2;
      if (vstart[mid] <= i) lo = mid; else hi = mid;
    }
    const u64 n = rstart[lo + 1] - rstart[lo];
    const u64 k = i - vstart[lo];
    const u64* col = reinterpret_cast<const u64*>(buf + base[lo] + 36);
    const long long* loff = reinterpret_cast<const long long*>(col + 3 * n + 1);
    u64 rl = 0, rh = n;
    while (rh - rl > 1) {
      const u64 mid = (rl + rh) / 2;
      if (loff[mid] <= (long long)k) rl = mid; else rh = mid;
    }
    o_vbits[i] = col[4 * n + 2 + k];
    o_vrow[i] = (long long)(rstart[lo] + rl);
  }
}

// One workgroup per EN_UNIT bytes of one MRL1 file, walked like an MRC1 file as
// the stream t = file offset + 4 (dst % 16 == 4):
//   t = 4                   "MRL1"
//   t = 8 + 8 w             word w: n | nb | nv | code | hi[n] | lo[n] | key_off[n + 1] | list_off[n + 1] |
//                           list_val[nv]
//   t = 56 + 32 n + 8 nv    key bytes (8 mod 16 for even nv, a 16-byte boundary for odd nv)
// Words go out as 8-byte stores; key_off and list_off are rebased to the file's
// first row (off / loff: the n + 1 offsets of the whole sorted table, lval its
// lval_cap values).  Key bytes: bytes up to the first 16-byte boundary of the
// destination (only behind the words, at most 8), then as in the MRC1 files.
__global__ void __launch_bounds__(EN_T) mrl1_encode_kernel(const u64* __restrict__ hi, const u64* __restrict__ lo,
                                                           const long long* __restrict__ off,
                                                           const long long* __restrict__ loff,
                                                           const u64* __restrict__ lval, u64 lval_cap,
                                                           const u8* __restrict__ blob, u64 blob_cap,
                                                           const u64* __restrict__ dsts, const u64* __restrict__ rstart,
                                                           const u64* __restrict__ rows,
                                                           const u64* __restrict__ unit_start, u32 nfiles, u64 code) {
  const u64 c = blockIdx.x;
  u32 flo = 0, fhi = nfiles;
  while (fhi - flo > 1) {
    const u32 mid = (flo + fhi) / 2;
    if (unit_start[mid] <= c) flo = mid; else fhi = mid;
  }
  const u32 j = flo;
  const u64 n = rows[j], a = rstart[j];
  const u64 o0 = (u64)off[a];
  const u64 nb = (u64)off[a + n] - o0;
  const u64 l0 = (u64)loff[a];
  const u64 nv = (u64)loff[a + n] - l0;
  const u64 tk = 56 + 32 * n + 8 * nv;  // stream position of the key bytes
  const u64 tend = tk + nb;             // ... and of the file's end
  const u64 t0 = (c - unit_start[j]) * EN_UNIT;
  if (t0 >= tend) return;
  const u64 t1 = t0 + EN_UNIT < tend ? t0 + EN_UNIT : tend;
  u8* base = reinterpret_cast<u8*>(dsts[j]) - 4;  // stream position 0: a 16-byte boundary
  const u32 t = threadIdx.x;
  if (t0 == 0 && t == 0) *reinterpret_cast<u32*>(base + 4) = 0x314C524Du;  // "MRL1"
  if (t0 < tk) {
    const u64 w0 = t0 ? (t0 - 8) / 8 : 0;
    const u64 w1 = ((t1 < tk ? t1 : tk) - 8) / 8;
    u64* dw = reinterpret_cast<u64*>(base + 8);
    for (u64 w = w0 + t; w < w1; w += EN_T) {
      u64 v;
      if (w < 4) v = w == 0 ? n : w == 1 ? nb : w == 2 ? nv : code;
      else if (w < 4 + n) v = hi[a + (w - 4)];
      else if (w < 4 + 2 * n) v = lo[a + (w - 4 - n)];
      else if (w < 5 + 3 * n) v = (u64)off[a + (w - 4 - 2 * n)] - o0;
      else if (w < 6 + 4 * n) v = (u64)loff[a + (w - 5 - 3 * n)] - l0;
      else {
        const u64 p = l0 + (w - 6 - 4 * n);
        v = p < lval_cap ? lval[p] : 0;
      }
      dw[w] = v;
    }
  }
  if (t1 > tk) {
    const u64 b0 = (t0 > tk ? t0 : tk) - tk, b1 = t1 - tk;  // key bytes [b0, b1) of the file
    u8* d = base + tk + b0;
    u64 head = (16 - ((tk + b0) & 15)) & 15;  // != 0 only when b0 == 0: every later unit starts on a boundary
    if (head > b1 - b0) head = b1 - b0;
    if (t < head) {
      const u64 p = o0 + b0 + t;
      d[t] = p < blob_cap ? blob[p] : (u8)0;
    }
    put_key_bytes(d + head, blob, blob_cap, o0 + b0 + head, b1 - b0 - head, t);
  }
}

}  // namespace mr

using namespace mr;

extern "C" {

int mr_ipc_alloc(unsigned long long nbytes, void** out) {
  *out = nullptr;
  return (int)hipMalloc(out, nbytes ? nbytes : 1);
}

int mr_ipc_free(void* p) { return p ? (int)hipFree(p) : 0; }

int mr_ipc_handle(void* p, void* out64) {
  hipIpcMemHandle_t h;
  const hipError_t e = hipIpcGetMemHandle(&h, p);
  if (e != hipSuccess) return (int)e;
  static_assert(sizeof(h) == 64, "hipIpcMemHandle_t is 64 bytes");
  std::memcpy(out64, &h, sizeof(h));
  return 0;
}

int mr_ipc_open(const void* handle64, void** out) {
  hipIpcMemHandle_t h;
  std::memcpy(&h, handle64, sizeof(h));
  *out = nullptr;
  return (int)hipIpcOpenMemHandle(out, h, hipIpcMemLazyEnablePeerAccess);
}

int mr_ipc_close(void* p) { return p ? (int)hipIpcCloseMemHandle(p) : 0; }

// table = device u64 [4 * n]: srcs | dsts | lens | chunk_start (the launch's
// copy list, uploaded by the caller); nchunks = chunk_start[n - 1] + chunks of
// the last copy
int mr_gather_copy(const void* table, unsigned n, unsigned long long nchunks, hipStream_t s) {
  if (n == 0 || nchunks == 0) return 0;
  const u64* t = static_cast<const u64*>(table);
  hipLaunchKernelGGL(gather_copy_kernel, dim3((unsigned)nchunks), dim3(GC_T), 0, s, t, t + n, t + 2 * n, t + 3 * n, n);
  return (int)hipGetLastError();
}

unsigned long long mr_gather_copy_chunk() { return GC_CHUNK; }

// meta = device u64 [2 * nfiles + 1]: base[nfiles] | rstart[nfiles + 1]
int mr_mrc1_decode(const void* buf, const void* meta, unsigned nfiles, unsigned long long nrows, void* hi, void* lo,
                   void* val, void* rep, hipStream_t s) {
  if (nrows == 0 || nfiles == 0) return 0;
  const u64* m = static_cast<const u64*>(meta);
  const u64 g = (nrows + DC_T - 1) / DC_T;
  hipLaunchKernelGGL(mrc1_decode_kernel, dim3((unsigned)g), dim3(DC_T), 0, s, (const u8*)buf, m, m + nfiles, nfiles,
                     nrows, (u64*)hi, (u64*)lo, (long long*)val, (u64*)rep);
  return (int)hipGetLastError();
}

// out = device i64 [2 * nparts + 4] (mrc1_plan_kernel); counts = the tail's
// partition counts, off = its n + 1 sorted key offsets, bad / err = its flags
int mr_mrc1_plan(const void* counts, const void* off, unsigned long long n, unsigned nparts, const void* bad,
                 const void* err, void* out, hipStream_t s) {
  if (nparts == 0 || nparts > (unsigned)PL_T) return -1;
  hipLaunchKernelGGL(mrc1_plan_kernel, dim3(1), dim3(PL_T), 0, s, (const long long*)counts, (const long long*)off,
                     (u64)n, nparts, (const u32*)bad, (const u32*)err, (long long*)out);
  return (int)hipGetLastError();
}

unsigned long long mr_mrc1_encode_unit() { return EN_UNIT; }

// workgroups (units) of a file of file_bytes bytes: its stream starts 4 bytes
// before the file, on a 16-byte boundary
unsigned long long mr_mrc1_encode_units(unsigned long long file_bytes) {
  return (file_bytes + 4 + EN_UNIT - 1) / EN_UNIT;
}

// plan = device u64 [4 * nfiles]: dst | row_start | rows | unit_start (the
// launch's file list, uploaded by the caller; dst % 16 == 4, file j = rows
// [row_start, row_start + rows) of the sorted columns); nunits = unit_start of
// the last file + its units.  Every file of a map job in ONE launch.
int mr_mrc1_encode(const void* hi, const void* lo, const void* val, const void* off, const void* blob,
                   unsigned long long blob_cap, const void* plan, unsigned nfiles, unsigned long long nunits,
                   hipStream_t s) {
  if (nfiles == 0 || nunits == 0) return 0;
  const u64* p = static_cast<const u64*>(plan);
  hipLaunchKernelGGL(mrc1_encode_kernel, dim3((unsigned)nunits), dim3(EN_T), 0, s, (const u64*)hi, (const u64*)lo,
                     (const u64*)val, (const long long*)off, (const u8*)blob, (u64)blob_cap, p, p + nfiles,
                     p + 2 * nfiles, p + 3 * nfiles, nfiles);
  return (int)hipGetLastError();
}

static bool mrc2_cols_ok(const Mrc2Cols* cs) {
  if (cs == nullptr || cs->k < 1 || cs->k > (u32)MRC2_MAXK) return false;
  for (u32 c = 0; c < cs->k; ++c)
    if (cs->code[c] > 2 || cs->col[c] == nullptr) return false;
  return true;
}

// meta as for mr_mrc1_decode; cols = host Mrc2Cols: the k output columns (i64 /
// f64 / f32 [nrows]) and the dtype codes every file has.  -1: k or a code the
// kernels do not know.
int mr_mrc2_decode(const void* buf, const void* meta, unsigned nfiles, unsigned long long nrows, void* hi, void* lo,
                   void* rep, const void* cols, hipStream_t s) {
  if (nrows == 0 || nfiles == 0) return 0;
  const Mrc2Cols* cs = static_cast<const Mrc2Cols*>(cols);
  if (!mrc2_cols_ok(cs)) return -1;
  const u64* m = static_cast<const u64*>(meta);
  const u64 g = (nrows + DC_T - 1) / DC_T;
  hipLaunchKernelGGL(mrc2_decode_kernel, dim3((unsigned)g), dim3(DC_T), 0, s, (const u8*)buf, m, m + nfiles, nfiles,
                     nrows, (u64*)hi, (u64*)lo, (u64*)rep, *cs);
  return (int)hipGetLastError();
}

unsigned long long mr_mrc2_encode_unit() { return EN_UNIT; }

// plan as for mr_mrc1_encode (a file of n rows and nb key bytes has
// 44 + 24 n + n * (sum of the widths) + nb bytes and ceil((bytes + 4) / unit)
// units); cols = host Mrc2Cols: the k sorted value columns and their codes.
int mr_mrc2_encode(const void* hi, const void* lo, const void* off, const void* blob, unsigned long long blob_cap,
                   const void* cols, const void* plan, unsigned nfiles, unsigned long long nunits, hipStream_t s) {
  if (nfiles == 0 || nunits == 0) return 0;
  const Mrc2Cols* cs = static_cast<const Mrc2Cols*>(cols);
  if (!mrc2_cols_ok(cs)) return -1;
  const u64* p = static_cast<const u64*>(plan);
  hipLaunchKernelGGL(mrc2_encode_kernel, dim3((unsigned)nunits), dim3(EN_T), 0, s, (const u64*)hi, (const u64*)lo,
                     (const long long*)off, (const u8*)blob, (u64)blob_cap, p, p + nfiles, p + 2 * nfiles,
                     p + 3 * nfiles, nfiles, *cs);
  return (int)hipGetLastError();
}

// out = device i64 [3 * nparts + 3] (mrl1_plan_kernel); counts = order_lists'
// partition counts, off / loff = its n + 1 sorted key and list offsets
int mr_mrl1_plan(const void* counts, const void* off, const void* loff, unsigned long long n, unsigned nparts,
                 void* out, hipStream_t s) {
  if (nparts == 0 || nparts > (unsigned)PL_T) return -1;
  hipLaunchKernelGGL(mrl1_plan_kernel, dim3(1), dim3(PL_T), 0, s, (const long long*)counts, (const long long*)off,
                     (const long long*)loff, (u64)n, nparts, (long long*)out);
  return (int)hipGetLastError();
}

unsigned long long mr_mrl1_encode_unit() { return EN_UNIT; }

// plan as for mr_mrc1_encode (a file of n rows, nv values and nb key bytes has
// 52 + 32 n + 8 nv + nb bytes and ceil((bytes + 4) / unit) units); loff / lval =
// the sorted table's n + 1 list offsets and its lval_cap values (8-byte words);
// code = what the files' headers say of them (0 = i64, 1 = f64).
int mr_mrl1_encode(const void* hi, const void* lo, const void* off, const void* loff, const void* lval,
                   unsigned long long lval_cap, const void* blob, unsigned long long blob_cap, const void* plan,
                   unsigned nfiles, unsigned long long nunits, unsigned code, hipStream_t s) {
  if (nfiles == 0 || nunits == 0) return 0;
  if (code > 1) return -1;
  const u64* p = static_cast<const u64*>(plan);
  hipLaunchKernelGGL(mrl1_encode_kernel, dim3((unsigned)nunits), dim3(EN_T), 0, s, (const u64*)hi, (const u64*)lo,
                     (const long long*)off, (const long long*)loff, (const u64*)lval, (u64)lval_cap, (const u8*)blob,
                     (u64)blob_cap, p, p + nfiles, p + 2 * nfiles, p + 3 * nfiles, nfiles, (u64)code);
  return (int)hipGetLastError();
}

// meta = device u64 [3 * nfiles + 2]: base[nfiles] | rstart[nfiles + 1] |
// vstart[nfiles + 1] (prefixes of the files' row and value counts); hi / lo /
// rep = [nrows], vbits / vrow = [nvals] (nvals may be 0 with rows present)
int mr_mrl1_decode(const void* buf, const void* meta, unsigned nfiles, unsigned long long nrows,
                   unsigned long long nvals, void* hi, void* lo, void* rep, void* vbits, void* vrow, hipStream_t s) {
  if (nrows == 0 || nfiles == 0) return 0;
  const u64* m = static_cast<const u64*>(meta);
  const u64 top = nrows > nvals ? nrows : nvals;
  const u64 g = (top + DC_T - 1) / DC_T;
  hipLaunchKernelGGL(mrl1_decode_kernel, dim3((unsigned)g), dim3(DC_T), 0, s, (const u8*)buf, m, m + nfiles,
                     m + 2 * nfiles + 1, nfiles, (u64)nrows, (u64)nvals, (u64*)hi, (u64*)lo, (u64*)rep, (u64*)vbits,
                     (long long*)vrow);
  return (int)hipGetLastError();
}

}  // extern "C"
