// pack.cpp — fixed-width packing of the input splits for the host->HBM link.
//
// A split of text uses few distinct byte values (the benchmark corpus: 59), so
// most of the bits that cross PCIe every iteration are padding.  Once a store
// has finished loading, every split is re-coded to k-bit codes (k = the
// smallest width in 1..7 that holds its alphabet); the packed copy is what an
// iteration ships, and a device kernel (csrc/hip/unpack.hip) restores the
// original bytes in the arena.  A split with more than 128 distinct values
// stays raw (k = 8): no table, no packed bytes.
//
// Layout of a packed split: groups of 16 symbols, each group 2k bytes, symbol i
// of a group in bits [k*i, k*i + k) of the group read as a little-endian
// integer; the last group is zero-padded.  Codes are assigned in ascending
// byte order (table[code] = byte, 128 bytes per split, unused entries 0).
// Every packed split starts at a 16-byte-aligned offset.
//
//   total = mrh_pack_plan(n, buf, off, nthreads, poff, pbytes, k, tables)
//       split i is buf[off[i], off[i+1]); fills poff[i] (16-aligned), pbytes[i]
//       (= ceil(len/16) * 2k, 0 for a raw split), k[i] and tables[128*i ..];
//       returns the size of the packed buffer, or -1 on bad arguments.
//   mrh_pack_run(n, buf, off, poff, k, tables, out, nthreads) -> 0
//       writes every packed split to out + poff[i] (the alignment gaps between
//       splits are left untouched: they are never read as symbols).
//
// Splits are handled in parallel by min(nthreads, 16, n) threads.
#include <atomic>
#include <cstdint>
#include <cstring>
#include <thread>
#include <vector>

namespace {

constexpr int kMaxThreads = 16;
constexpr int kTable = 128;

template <class F>
void for_each_split(int n, int nthreads, F fn) {
  if (nthreads < 1) nthreads = 1;
  if (nthreads > kMaxThreads) nthreads = kMaxThreads;
  if (nthreads > n) nthreads = n;
  std::atomic<int> next{0};
  auto work = [&] {
    for (;;) {
      const int i = next.fetch_add(1, std::memory_order_relaxed);
      if (i >= n) break;
      fn(i);
    }
  };
  if (nthreads <= 1) {
    work();
    return;
  }
  std::vector<std::thread> th;
  for (int t = 0; t < nthreads; ++t) th.emplace_back(work);
  for (auto& t : th) t.join();
}

// alphabet of one split: width, and the code table in ascending byte order
int scan_split(const uint8_t* p, int64_t len, uint8_t* table) {
  uint64_t hist[4][256];
  memset(hist, 0, sizeof hist);
  int64_t i = 0;
  for (; i + 4 <= len; i += 4) {
    ++hist[0][p[i]];
    ++hist[1][p[i + 1]];
    ++hist[2][p[i + 2]];
    ++hist[3][p[i + 3]];
  }
  for (; i < len; ++i) ++hist[0][p[i]];
  int a = 0;
  for (int b = 0; b < 256; ++b) a += (hist[0][b] | hist[1][b] | hist[2][b] | hist[3][b]) != 0;
  memset(table, 0, kTable);
  if (a > kTable) return 8;
  int code = 0;
  for (int b = 0; b < 256; ++b)
    if (hist[0][b] | hist[1][b] | hist[2][b] | hist[3][b]) table[code++] = (uint8_t)b;
  int k = 1;
  while ((1 << k) < a) ++k;
  return k;
}

void pack_split(const uint8_t* p, int64_t len, int k, const uint8_t* table, uint8_t* out) {
  uint8_t code[256];
  memset(code, 0, sizeof code);
  // descending: the unused entries (byte 0) are written first, so byte 0 —
  // code 0 whenever it is in the alphabet — ends with its own code
  for (int c = (1 << k) - 1; c >= 0; --c) code[table[c]] = (uint8_t)c;
  const int gb = 2 * k;
  int64_t i = 0;
  for (; i + 16 <= len; i += 16, out += gb) {
    unsigned __int128 acc = 0;
    for (int j = 0; j < 16; ++j) acc |= (unsigned __int128)code[p[i + j]] << (k * j);
    const uint64_t lo = (uint64_t)acc, hi = (uint64_t)(acc >> 64);
    uint8_t tmp[16];
    memcpy(tmp, &lo, 8);
    memcpy(tmp + 8, &hi, 8);
    memcpy(out, tmp, gb);
  }
  if (i < len) {
    unsigned __int128 acc = 0;
    for (int j = 0; i + j < len; ++j) acc |= (unsigned __int128)code[p[i + j]] << (k * j);
    const uint64_t lo = (uint64_t)acc, hi = (uint64_t)(acc >> 64);
    uint8_t tmp[16];
    memcpy(tmp, &lo, 8);
    memcpy(tmp + 8, &hi, 8);
    memcpy(out, tmp, gb);
  }
}

}  // namespace

extern "C" {

int64_t mrh_pack_plan(int n, const uint8_t* buf, const int64_t* off, int nthreads, int64_t* poff, int64_t* pbytes,
                      int32_t* k, uint8_t* tables) {
  if (n < 0 || !off || !poff || !pbytes || !k || !tables || (n > 0 && !buf)) return -1;
  for (int i = 0; i < n; ++i)
    if (off[i + 1] < off[i]) return -1;
  for_each_split(n, nthreads, [&](int i) { k[i] = scan_split(buf + off[i], off[i + 1] - off[i], tables + kTable * i); });
  int64_t at = 0;
  for (int i = 0; i < n; ++i) {
    const int64_t len = off[i + 1] - off[i];
    poff[i] = at;
    pbytes[i] = k[i] == 8 ? 0 : (len + 15) / 16 * 2 * k[i];
    at += (pbytes[i] + 15) & ~(int64_t)15;
  }
  return at;
}

int mrh_pack_run(int n, const uint8_t* buf, const int64_t* off, const int64_t* poff, const int32_t* k,
                 const uint8_t* tables, uint8_t* out, int nthreads) {
  if (n < 0 || !off || !poff || !k || !tables || (n > 0 && (!buf || !out))) return -1;
  for_each_split(n, nthreads, [&](int i) {
    if (k[i] >= 1 && k[i] <= 7) pack_split(buf + off[i], off[i + 1] - off[i], k[i], tables + kTable * i, out + poff[i]);
  });
  return 0;
}

}  // extern "C"
