// undict.hip — restores the original bytes of dictionary-coded input splits in
// the HBM arena (the device half of csrc/host/dictpack.cpp).
//
// The host store ships a split as little-endian u16 code units: a unit
// u < 0xC000 is dictionary entry u; a unit u >= 0xC000 is a lead, followed by
// one unit v < 0xC000, and the two name entry 0xC000 + (u - 0xC000) * 0xC000 + v.
// Unit i is a continuation iff unit i-1 is >= 0xC000, so every lane decides that
// on its own.  The dictionary lives in HBM: one 32-byte slot per entry, bytes
// 0..30 the entry, byte 31 its length.  A tile index per split (rows of {u32
// first unit, u32 first output byte}, one closing row behind the last tile)
// cuts the stream at code boundaries into tiles of at most 4096 units and at
// most 8192 output bytes.
//
// Work split: blockIdx.y = descriptor (one split), blockIdx.x = tile.  A
// workgroup loads its units into LDS, looks up the entry lengths (unit
// i = lane + 256 j: neighbouring lanes hold neighbouring codes), scans them
// block-wide, ORs the entry bytes as whole dwords into a zeroed LDS image of
// the tile laid out with the destination's residue mod 16, and copies the
// image out: interior 16-byte slots as 16-byte stores, the ragged first and
// last slot with byte stores — neighbouring tiles and splits are written by
// other workgroups at the same time.  Every access is bounded by the buffer sizes, the tile's unit count
// and its output range: a code that does not fit (entry beyond the dictionary,
// a lead as a tile's last unit, bytes past the tile's end) writes nothing.
#include <hip/hip_runtime.h>

#include "mr_common.h"

namespace {

struct UndictDesc {
  u64 src;     // byte offset of the split's units in the staging buffer (16-aligned)
  u64 dst;     // byte offset of the split in the arena
  u32 n;       // bytes of the split
  u32 units;   // code units of the split
  u32 tix;     // first row of the split's tile index
  u32 ntiles;  // tiles of the split (the index has ntiles + 1 rows)
};

constexpr int UD_THREADS = 256;
constexpr int UD_PER = 16;  // units per thread
constexpr u32 UD_TILE_UNITS = UD_THREADS * UD_PER;
constexpr u32 UD_TILE_BYTES = 8192;
constexpr u32 UD_LEAD = 0xC000u;
constexpr u32 UD_NONE = 0xFFFFFFFFu;
constexpr u32 UD_MAX_Y = 65535;

__global__ __launch_bounds__(UD_THREADS) void undict_splits_kernel(const u8* __restrict__ staging, u64 staging_bytes,
                                                                    u8* __restrict__ arena, u64 arena_bytes,
                                                                    const UndictDesc* __restrict__ desc,
                                                                    const uint2* __restrict__ tix, u64 tix_rows,
                                                                    const uint4* __restrict__ dict, u32 entries) {
  __shared__ __attribute__((aligned(16))) u16 su[UD_TILE_UNITS];   // units, then the codes' output offsets
  __shared__ __attribute__((aligned(16))) u8 slen[UD_TILE_UNITS];  // output bytes of the code that starts at unit i
  __shared__ __attribute__((aligned(16))) u8 sout[UD_TILE_BYTES + 16];
  __shared__ u32 swave[UD_THREADS / 64];

  const UndictDesc d = desc[blockIdx.y];
  const u32 t = blockIdx.x;
  // a descriptor or tile that does not fit its buffers is skipped whole (the
  // host validates the plan; this keeps a bad one from writing out of bounds)
  if (t >= d.ntiles || (u64)d.tix + t + 1 >= tix_rows || d.dst > arena_bytes || d.n > arena_bytes - d.dst ||
      d.src > staging_bytes || 2ull * d.units > staging_bytes - d.src)
    return;
  const uint2 row = tix[(u64)d.tix + t], end = tix[(u64)d.tix + t + 1];
  const u32 u0 = row.x, b0 = row.y;
  if (end.x < u0 || end.x > d.units || end.x - u0 > UD_TILE_UNITS || end.y < b0 || end.y > d.n ||
      end.y - b0 > UD_TILE_BYTES)
    return;
  const u32 nu = end.x - u0, nb = end.y - b0;
  if (nb == 0) return;
  const u32 tid = threadIdx.x;
  const u16* const src = reinterpret_cast<const u16*>(staging + d.src) + u0;

  for (u32 i = tid; i < UD_TILE_UNITS; i += UD_THREADS) su[i] = i < nu ? src[i] : (u16)0;
  for (u32 i = tid; i < (UD_TILE_BYTES + 16) / 16; i += UD_THREADS)
    reinterpret_cast<uint4*>(sout)[i] = make_uint4(0, 0, 0, 0);
  __syncthreads();

  // A: entry and length of the code that starts at unit i = tid + 256 j
  u32 ent[UD_PER];
#pragma unroll
  for (int j = 0; j < UD_PER; ++j) {
    const u32 i = tid + UD_THREADS * j;
    u32 e = UD_NONE;
    if (i < nu && !(i > 0 && su[i - 1] >= UD_LEAD)) {
      const u32 u = su[i];
      if (u < UD_LEAD) {
        e = u;
      } else if (i + 1 < nu && su[i + 1] < UD_LEAD) {
        e = UD_LEAD + (u - UD_LEAD) * UD_LEAD + su[i + 1];
      }
      if (e >= entries) e = UD_NONE;
    }
    u32 len = 0;
    if (e != UD_NONE) {
      len = reinterpret_cast<const u8*>(dict + 2ull * e)[31];
      if (len > 31) len = 31;
    }
    ent[j] = e;
    slen[i] = (u8)len;
  }
  __syncthreads();

  // B: exclusive scan of the lengths in unit order; thread tid owns units 16 tid .. 16 tid + 15
  {
    const uint4 l4 = *reinterpret_cast<const uint4*>(slen + UD_PER * tid);
    const u32 lw[4] = {l4.x, l4.y, l4.z, l4.w};
    u32 pre[UD_PER];
    u32 sum = 0;
#pragma unroll
    for (int k = 0; k < UD_PER; ++k) {
      pre[k] = sum;
      sum += (lw[k >> 2] >> (8 * (k & 3))) & 0xFFu;
    }
    u32 inc = sum;  // inclusive scan over the wave
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
      const u32 v = __shfl_up(inc, o, 64);
      if ((tid & 63) >= (u32)o) inc += v;
    }
    if ((tid & 63) == 63) swave[tid >> 6] = inc;
    __syncthreads();  // (also: every thread has read its units of su in A)
    u32 base = inc - sum;
    for (u32 w = 0; w < (tid >> 6); ++w) base += swave[w];
#pragma unroll
    for (int k = 0; k < UD_PER; ++k) {
      const u32 o = base + pre[k];
      su[UD_PER * tid + k] = (u16)(o < 0xFFFFu ? o : 0xFFFFu);  // (a bad stream: 4096 x 31 bytes overflow 16 bits)
    }
  }
  __syncthreads();

  // C: entry bytes into the LDS image; byte b of the tile is sout[r + b].  A code ORs its bytes in as whole dwords
  // (the image starts as zeros and a slot is zero behind its entry), so neighbouring codes share dwords safely
  u8* const dst = arena + d.dst + b0;
  const u32 r = (u32)(reinterpret_cast<uintptr_t>(dst) & 15u);
  u32* const simg = reinterpret_cast<u32*>(sout);
#pragma unroll
  for (int j = 0; j < UD_PER; ++j) {
    const u32 e = ent[j];
    if (e == UD_NONE) continue;
    const u32 i = tid + UD_THREADS * j;
    const u32 o = su[i], len = slen[i];
    if (len == 0 || o + len > nb) continue;
    const uint4 a = dict[2ull * e], b = dict[2ull * e + 1];
    const u32 w[8] = {a.x, a.y, a.z, a.w, b.x, b.y, b.z, b.w & 0x00FFFFFFu};  // (byte 31 is the length)
    const u32 pos = r + o, sh = 8 * (pos & 3u), nd = ((pos & 3u) + len + 3) >> 2;  // dwords touched: 1..9
    u32 prev = 0;
#pragma unroll
    for (int k = 0; k < 9; ++k) {
      if ((u32)k < nd) {
        const u32 cur = k < 8 ? w[k < 8 ? k : 0] : 0u;
        const u32 v = sh ? (cur << sh) | (prev >> (32 - sh)) : cur;
        atomicOr(&simg[(pos >> 2) + k], v);
        prev = cur;
      }
    }
  }
  __syncthreads();

  // D: copy out; slot s is the 16 aligned destination bytes [base + 16 s, base + 16 s + 16)
  u8* const base = dst - r;  // bytes before dst are never touched
  const u32 nslots = (r + nb + 15) >> 4;
  for (u32 s = tid; s < nslots; s += UD_THREADS) {
    const u32 lo = s == 0 ? r : 0u;
    const u32 left = r + nb - 16 * s;
    const u32 hi = left < 16 ? left : 16u;
    if (lo == 0 && hi == 16) {
      *reinterpret_cast<uint4*>(base + 16ull * s) = *reinterpret_cast<const uint4*>(sout + 16 * s);
    } else {
      for (u32 k = lo; k < hi; ++k) base[16ull * s + k] = sout[16 * s + k];
    }
  }
}

}  // namespace

extern "C" {

// Decode `ndesc` dictionary-coded splits (device descriptors: 32 bytes each,
// {u64 src, u64 dst, u32 n, u32 units, u32 tix, u32 ntiles}) from `staging`
// into `arena`; `max_tiles` is the largest tile count among them (it sizes the
// grid).  `tix` holds `tix_rows` rows of the tile indexes, `dict` `entries`
// 32-byte slots.  The staging buffer and every src are 16-byte aligned, the
// dictionary 32-byte; the sizes bound every access.
int mr_undict_splits(const void* staging, u64 staging_bytes, void* arena, u64 arena_bytes, const void* desc, u64 ndesc,
                     u64 max_tiles, const void* tix, u64 tix_rows, const void* dict, u64 entries, hipStream_t s) {
  if (ndesc == 0 || max_tiles == 0) return 0;
  if ((reinterpret_cast<uintptr_t>(staging) & 15u) != 0 || (reinterpret_cast<uintptr_t>(dict) & 31u) != 0 ||
      (reinterpret_cast<uintptr_t>(tix) & 7u) != 0 || max_tiles > 0x7FFFFFFFull || entries > 0xFFFFFFFFull)
    return (int)hipErrorInvalidValue;
  const UndictDesc* d = static_cast<const UndictDesc*>(desc);
  for (u64 at = 0; at < ndesc; at += UD_MAX_Y) {
    const u32 ny = (u32)(ndesc - at < UD_MAX_Y ? ndesc - at : UD_MAX_Y);
    hipLaunchKernelGGL(undict_splits_kernel, dim3((u32)max_tiles, ny), dim3(UD_THREADS), 0, s, (const u8*)staging,
                       staging_bytes, (u8*)arena, arena_bytes, d + at, (const uint2*)tix, tix_rows, (const uint4*)dict,
                       (u32)entries);
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) return (int)e;
  }
  return 0;
}

}  // extern "C"
