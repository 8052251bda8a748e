// unpack.hip — restores the original bytes of bit-packed input splits in the
// HBM arena (the device half of csrc/host/pack.cpp).
//
// The host store ships every split as fixed-width k-bit codes (k = 1..7, groups
// of 16 symbols = 2k bytes, little-endian bit order, one 128-byte code table per
// split); the copy engine lands them in a device staging buffer and ONE launch
// of this kernel per chunk of splits writes the original bytes to the splits'
// places in the arena, so everything downstream (map kernels, key-byte reads,
// the tail) sees the arena it has always seen.
//
// Work split: blockIdx.y = descriptor (one split), blockIdx.x = a tile of
// 16-byte-ALIGNED destination slots.  A split's destination is an arbitrary
// byte offset, so an aligned slot holds the tail of group s-1 and the head of
// group s: a lane decodes both (the decode is a handful of bit-field extracts
// and LDS table reads, far below the memory time) and funnels them into one
// 16-byte store.  The first and last slot of a split are ragged: only their
// bytes inside [dst, dst + n) are written, with byte stores — neighbouring
// splits are written by other workgroups at the same time.
#include <hip/hip_runtime.h>

#include "mr_common.h"

namespace {

struct UnpackDesc {
  u64 src;  // byte offset of the packed split in the staging buffer (16-aligned)
  u64 dst;  // byte offset of the split in the arena
  u64 n;    // bytes of the split
  u32 k;    // code width, 1..7
  u32 tab;  // byte offset of the split's 128-byte code table
};

constexpr int UNPACK_THREADS = 256;
constexpr int UNPACK_SLOTS = 4;  // 16-byte slots per thread
constexpr u64 UNPACK_TILE_SLOTS = (u64)UNPACK_THREADS * UNPACK_SLOTS;
constexpr u32 UNPACK_MAX_Y = 65535;

typedef unsigned __int128 u128;

// One group: 2K packed bytes -> 16 bytes.  K even: dword loads (2K * g is a
// multiple of 4 from a 16-aligned start); K odd: 16-bit loads.
template <int K>
__device__ __forceinline__ u128 decode_group(const u8* __restrict__ g, const u8* tab) {
  u32 w[4] = {0u, 0u, 0u, 0u};
  if constexpr (K % 2 == 0) {
    const u32* p = reinterpret_cast<const u32*>(g);
#pragma unroll
    for (int i = 0; i < K / 2; ++i) w[i] = p[i];
  } else {
    const u16* p = reinterpret_cast<const u16*>(g);
#pragma unroll
    for (int i = 0; i < K; ++i) w[i >> 1] |= (u32)p[i] << (16 * (i & 1));
  }
  u32 o[4] = {0u, 0u, 0u, 0u};
#pragma unroll
  for (int i = 0; i < 16; ++i) {
    constexpr u32 mask = (1u << K) - 1u;
    const int bit = K * i, wd = bit >> 5, sh = bit & 31;
    u32 c = w[wd] >> sh;
    if (sh + K > 32) c |= w[wd + 1] << (32 - sh);  // bit < 112: wd + 1 <= 3
    o[i >> 2] |= (u32)tab[c & mask] << (8 * (i & 3));
  }
  return (u128)o[0] | ((u128)o[1] << 32) | ((u128)o[2] << 64) | ((u128)o[3] << 96);
}

template <int K>
__device__ __forceinline__ void unpack_tile(const u8* __restrict__ src, u8* __restrict__ dst, u64 n, const u8* tab,
                                            u64 tile) {
  const u32 r = (u32)(reinterpret_cast<uintptr_t>(dst) & 15u);
  u8* const base = dst - r;  // 16-aligned; bytes before dst are never touched
  const u64 nslots = (r + n + 15) >> 4;
  const u64 ngroups = (n + 15) >> 4;
#pragma unroll
  for (int u = 0; u < UNPACK_SLOTS; ++u) {
    const u64 s = tile * UNPACK_TILE_SLOTS + (u64)u * UNPACK_THREADS + threadIdx.x;
    if (s >= nslots) break;
    // slot byte j holds symbol 16 s + j - r: j < r from group s-1, the rest from group s
    u128 out = s < ngroups ? decode_group<K>(src + (u64)(2 * K) * s, tab) : (u128)0;
    if (r != 0) {
      const u128 prev = s > 0 ? decode_group<K>(src + (u64)(2 * K) * (s - 1), tab) : (u128)0;  // s - 1 < ngroups
      out = (prev >> (8 * (16 - r))) | (out << (8 * r));
    }
    const u32 lo = s == 0 ? r : 0u;
    const u64 left = r + n - 16 * s;  // slot bytes up to the split's end
    const u32 hi = left < 16 ? (u32)left : 16u;
    u8* const p = base + 16 * s;
    if (lo == 0 && hi == 16) {
      uint4 v;
      v.x = (u32)out;
      v.y = (u32)(out >> 32);
      v.z = (u32)(out >> 64);
      v.w = (u32)(out >> 96);
      *reinterpret_cast<uint4*>(p) = v;
    } else {
      for (u32 j = lo; j < hi; ++j) p[j] = (u8)(out >> (8 * j));
    }
  }
}

__global__ __launch_bounds__(UNPACK_THREADS) void unpack_splits_kernel(const u8* __restrict__ staging,
                                                                        u64 staging_bytes, u8* __restrict__ arena,
                                                                        u64 arena_bytes,
                                                                        const UnpackDesc* __restrict__ desc,
                                                                        const u8* __restrict__ tables,
                                                                        u64 tables_bytes) {
  __shared__ u8 tab[128];
  const UnpackDesc d = desc[blockIdx.y];
  const u32 k = d.k;
  // a descriptor that does not fit its buffers is skipped whole (the host
  // validates the plan; this keeps a bad one from writing out of bounds)
  if (k < 1 || k > 7 || d.n == 0 || d.dst > arena_bytes || d.n > arena_bytes - d.dst || d.src > staging_bytes ||
      ((d.n + 15) >> 4) * 2 * k > staging_bytes - d.src || (u64)d.tab + 128 > tables_bytes)
    return;
  u8* const dst = arena + d.dst;
  const u32 r = (u32)(reinterpret_cast<uintptr_t>(dst) & 15u);
  const u64 tile = blockIdx.x;
  if (tile * UNPACK_TILE_SLOTS >= ((r + d.n + 15) >> 4)) return;
  if (threadIdx.x < 128) tab[threadIdx.x] = tables[d.tab + threadIdx.x];
  __syncthreads();
  const u8* const src = staging + d.src;
  switch (k) {
    case 1: unpack_tile<1>(src, dst, d.n, tab, tile); break;
    case 2: unpack_tile<2>(src, dst, d.n, tab, tile); break;
    case 3: unpack_tile<3>(src, dst, d.n, tab, tile); break;
    case 4: unpack_tile<4>(src, dst, d.n, tab, tile); break;
    case 5: unpack_tile<5>(src, dst, d.n, tab, tile); break;
    case 6: unpack_tile<6>(src, dst, d.n, tab, tile); break;
    default: unpack_tile<7>(src, dst, d.n, tab, tile); break;
  }
}

}  // namespace

extern "C" {

// Unpack `ndesc` splits (device descriptors: 32 bytes each, {u64 src, u64 dst,
// u64 n, u32 k, u32 tab}) from `staging` into `arena`; `max_n` is the largest
// split among them (it sizes the grid).  The staging buffer must be 16-byte
// aligned; the buffer sizes bound every access.
int mr_unpack_splits(const void* staging, u64 staging_bytes, void* arena, u64 arena_bytes, const void* desc, u64 ndesc,
                     u64 max_n, const void* tables, u64 tables_bytes, hipStream_t s) {
  if (ndesc == 0 || max_n == 0) return 0;
  if ((reinterpret_cast<uintptr_t>(staging) & 15u) != 0) return (int)hipErrorInvalidValue;
  const u64 tiles = (((15 + max_n + 15) >> 4) + UNPACK_TILE_SLOTS - 1) / UNPACK_TILE_SLOTS;
  if (tiles > 0x7FFFFFFFull) return (int)hipErrorInvalidValue;
  const UnpackDesc* d = static_cast<const UnpackDesc*>(desc);
  for (u64 at = 0; at < ndesc; at += UNPACK_MAX_Y) {
    const u32 ny = (u32)(ndesc - at < UNPACK_MAX_Y ? ndesc - at : UNPACK_MAX_Y);
    hipLaunchKernelGGL(unpack_splits_kernel, dim3((u32)tiles, ny), dim3(UNPACK_THREADS), 0, s, (const u8*)staging,
                       staging_bytes, (u8*)arena, arena_bytes, d + at, (const u8*)tables, tables_bytes);
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) return (int)e;
  }
  return 0;
}

}  // extern "C"
