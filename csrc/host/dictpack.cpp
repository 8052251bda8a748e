// dictpack.cpp — dictionary coding of the input splits for the host->HBM link.
//
// The fixed-width packer (pack.cpp) removes padding bits only; text also
// repeats a small set of words.  Here whole tokens are coded against one
// dictionary per store, which is uploaded to HBM once; an iteration ships
// 16-bit code units and a device kernel (csrc/hip/undict.hip) restores the
// original bytes in the arena.
//
// Token: a maximal run of non-whitespace bytes plus the one byte that follows
// it (whitespace: space \t \n \v \f \r).  A run at the very end of a split, with
// no byte behind it, is no token.  Tokens of 2..31 bytes are dictionary
// candidates.
//
// Dictionary: entries 0..255 are the single bytes (every input can be coded);
// the other entries are the candidates ranked by count * length, descending,
// ties by the entry's bytes (so the result does not depend on the thread
// count), at most 1 Mi entries in all.  Device layout: one 32-byte slot per
// entry, bytes 0..30 the entry (zero padded), byte 31 its length.
//
// Code stream: little-endian u16 units.  A unit u < 0xC000 is entry u.  A unit
// u >= 0xC000 is a lead and is followed by exactly one unit v < 0xC000; the two
// name entry 0xC000 + (u - 0xC000) * 0xC000 + v.  Unit i is a continuation if
// and only if unit i-1 is >= 0xC000.  A token that is in the dictionary is one
// code; every other byte (longer tokens, whitespace runs, a last run without a
// separator) is its single-byte code.
//
// Tile index of a split: rows of {u32 first unit, u32 first output byte}, both
// relative to the split; a tile starts on a code boundary and holds at most
// 4096 units and at most 8192 output bytes; one closing row {units, bytes}
// follows the last tile (tiles + 1 rows, one row for an empty split).
//
//   h = mrh_dict_build(n, buf, off, nthreads, max_entries)   split i is buf[off[i], off[i+1])
//   mrh_dict_entries(h) -> entries;  mrh_dict_slots(h, out) writes 32 * entries bytes
//   mrh_dict_plan(h, n, buf, off, nthreads, units, tiles) -> 0
//       encodes every split smaller than 4 GiB (kept in h); units[i] / tiles[i]
//       of split i (units[i] = -1: not coded)
//   mrh_dict_run(h, n, uoff, toff, out, tix, nthreads) -> 0
//       split i with uoff[i] >= 0: its units to out + uoff[i] (a byte offset,
//       even), its tiles[i] + 1 index rows to tix + 2 * toff[i]
//   mrh_dict_free(h)
//
// Splits are handled in parallel by min(nthreads, 16, n) threads.
#include <algorithm>
#include <atomic>
#include <cstdint>
#include <cstring>
#include <thread>
#include <vector>

namespace {

constexpr int kMaxThreads = 16;
constexpr int kMaxToken = 31;
constexpr uint32_t kLead = 0xC000u;
constexpr int64_t kMaxEntries = 1 << 20;
constexpr uint32_t kTileUnits = 4096, kTileBytes = 8192;

inline bool is_ws(uint8_t c) { return c == 32 || (uint8_t)(c - 9) < 5; }

// a token as its dictionary slot: bytes 0..30 zero padded, byte 31 the length
struct Key {
  uint64_t w[4];
  bool operator==(const Key& o) const { return w[0] == o.w[0] && w[1] == o.w[1] && w[2] == o.w[2] && w[3] == o.w[3]; }
};

inline Key make_key(const uint8_t* p, int len) {
  uint8_t b[32];
  memset(b, 0, sizeof b);
  memcpy(b, p, (size_t)len);
  b[31] = (uint8_t)len;
  Key k;
  memcpy(k.w, b, 32);
  return k;
}

inline uint64_t mix(uint64_t x) {
  x ^= x >> 33;
  x *= 0xff51afd7ed558ccdull;
  x ^= x >> 33;
  x *= 0xc4ceb9fe1a85ec53ull;
  x ^= x >> 33;
  return x;
}

inline uint64_t hash_key(const Key& k) {
  return mix(k.w[0] ^ mix(k.w[1] + 0x9E3779B97F4A7C15ull) ^ mix(k.w[2] + 0xC2B2AE3D27D4EB4Full) ^ mix(k.w[3] + 0x165667B19E3779F9ull));
}

// open addressing, linear probing; a slot with w[3] == 0 is empty (a key's
// length byte is never 0)
struct Table {
  struct Slot {
    Key k;
    uint64_t v;
  };
  std::vector<Slot> s;
  uint64_t used = 0;
  Table() { s.assign(1u << 12, Slot{{{0, 0, 0, 0}}, 0}); }
  void grow() {
    std::vector<Slot> old;
    old.swap(s);
    s.assign(old.size() * 2, Slot{{{0, 0, 0, 0}}, 0});
    for (const Slot& e : old)
      if (e.k.w[3]) *find(e.k) = e;
  }
  Slot* find(const Key& k) {
    const uint64_t m = s.size() - 1;
    for (uint64_t i = hash_key(k) & m;; i = (i + 1) & m)
      if (s[i].k.w[3] == 0 || s[i].k == k) return &s[i];
  }
  const Slot* find(const Key& k) const { return const_cast<Table*>(this)->find(k); }
  void add(const Key& k, uint64_t v) {
    Slot* e = find(k);
    if (e->k.w[3] == 0) {
      e->k = k;
      e->v = 0;
      if (++used * 10 > s.size() * 6) {
        grow();
        e = find(k);
      }
    }
    e->v += v;
  }
};

template <class F>
void parallel(int n, int nthreads, F fn) {  // fn(thread, item)
  if (nthreads < 1) nthreads = 1;
  if (nthreads > kMaxThreads) nthreads = kMaxThreads;
  if (nthreads > n) nthreads = n;
  std::atomic<int> next{0};
  auto work = [&](int t) {
    for (;;) {
      const int i = next.fetch_add(1, std::memory_order_relaxed);
      if (i >= n) break;
      fn(t, i);
    }
  };
  if (nthreads <= 1) {
    work(0);
    return;
  }
  std::vector<std::thread> th;
  for (int t = 0; t < nthreads; ++t) th.emplace_back(work, t);
  for (auto& t : th) t.join();
}

// calls fn(start, len) for every token of the split and fn(start, 0) for every
// byte outside a token, in order
template <class F>
inline void scan_tokens(const uint8_t* p, int64_t n, F fn) {
  int64_t i = 0;
  while (i < n) {
    if (is_ws(p[i])) {
      fn(i, (int64_t)0);
      ++i;
      continue;
    }
    int64_t e = i + 1;
    while (e < n && !is_ws(p[e])) ++e;
    if (e < n) {
      fn(i, e + 1 - i);
      i = e + 1;
    } else {  // a last run without a separator
      for (; i < n; ++i) fn(i, (int64_t)0);
    }
  }
}

struct Coded {
  std::vector<uint16_t> units;
  std::vector<uint32_t> rows;  // {first unit, first output byte} per tile, then the closing row
  bool done = false;
};

struct Dict {
  std::vector<Key> entries;  // entry index -> slot
  Table index;               // slot -> entry index (entries >= 256 only)
  std::vector<Coded> coded;
};

void encode_split(const Dict& d, const uint8_t* p, int64_t n, Coded& c) {
  c.units.clear();
  c.rows.clear();
  c.units.reserve((size_t)(n / 3 + 16));
  uint32_t tile_u = 0, tile_b = 0;  // start of the open tile
  bool open = false;
  auto emit = [&](uint32_t entry, uint32_t len, int64_t at) {
    const uint32_t nu = entry < kLead ? 1u : 2u;
    const uint32_t u = (uint32_t)c.units.size(), b = (uint32_t)at;
    if (!open || u + nu - tile_u > kTileUnits || b + len - tile_b > kTileBytes) {
      c.rows.push_back(u);
      c.rows.push_back(b);
      tile_u = u;
      tile_b = b;
      open = true;
    }
    if (nu == 1) {
      c.units.push_back((uint16_t)entry);
    } else {
      const uint32_t r = entry - kLead;
      c.units.push_back((uint16_t)(kLead + r / kLead));
      c.units.push_back((uint16_t)(r % kLead));
    }
  };
  scan_tokens(p, n, [&](int64_t at, int64_t len) {
    if (len >= 2 && len <= kMaxToken) {
      const Table::Slot* e = d.index.find(make_key(p + at, (int)len));
      if (e->k.w[3]) {
        emit((uint32_t)e->v, (uint32_t)len, at);
        return;
      }
    }
    if (len == 0) {
      emit(p[at], 1, at);
    } else {
      for (int64_t j = 0; j < len; ++j) emit(p[at + j], 1, at + j);
    }
  });
  c.rows.push_back((uint32_t)c.units.size());
  c.rows.push_back((uint32_t)n);
  c.done = true;
}

bool bad_splits(int n, const uint8_t* buf, const int64_t* off) {
  if (n < 0 || !off || (n > 0 && !buf)) return true;
  for (int i = 0; i < n; ++i)
    if (off[i + 1] < off[i]) return true;
  return false;
}

}  // namespace

extern "C" {

void* mrh_dict_build(int n, const uint8_t* buf, const int64_t* off, int nthreads, int64_t max_entries) {
  if (bad_splits(n, buf, off)) return nullptr;
  if (max_entries < 256) max_entries = 256;
  if (max_entries > kMaxEntries) max_entries = kMaxEntries;
  std::vector<Table> tabs(kMaxThreads);
  parallel(n, nthreads, [&](int t, int i) {
    const uint8_t* p = buf + off[i];
    Table& tab = tabs[t];
    scan_tokens(p, off[i + 1] - off[i], [&](int64_t at, int64_t len) {
      if (len >= 2 && len <= kMaxToken) tab.add(make_key(p + at, (int)len), 1);
    });
  });
  Table& all = tabs[0];
  for (int t = 1; t < kMaxThreads; ++t) {
    for (const Table::Slot& e : tabs[t].s)
      if (e.k.w[3]) all.add(e.k, e.v);
    std::vector<Table::Slot>().swap(tabs[t].s);
  }
  struct Cand {
    uint64_t score;
    Key k;
  };
  std::vector<Cand> cand;
  cand.reserve((size_t)all.used);
  for (const Table::Slot& e : all.s)
    if (e.k.w[3]) cand.push_back({e.v * (e.k.w[3] >> 56), e.k});  // (little-endian: byte 31 is the top byte of w[3])
  auto before = [](const Cand& a, const Cand& b) {
    if (a.score != b.score) return a.score > b.score;
    return memcmp(a.k.w, b.k.w, 32) < 0;
  };
  const size_t keep = std::min(cand.size(), (size_t)(max_entries - 256));
  std::partial_sort(cand.begin(), cand.begin() + (std::ptrdiff_t)keep, cand.end(), before);
  Dict* d = new Dict;
  d->entries.reserve(256 + keep);
  for (int b = 0; b < 256; ++b) {
    const uint8_t c = (uint8_t)b;
    d->entries.push_back(make_key(&c, 1));
  }
  for (size_t i = 0; i < keep; ++i) {
    d->entries.push_back(cand[i].k);
    d->index.add(cand[i].k, 256 + i);
  }
  return d;
}

int64_t mrh_dict_entries(void* h) { return h ? (int64_t) static_cast<Dict*>(h)->entries.size() : -1; }

int mrh_dict_slots(void* h, uint8_t* out) {
  if (!h || !out) return -1;
  const Dict* d = static_cast<Dict*>(h);
  memcpy(out, d->entries.data(), d->entries.size() * 32);
  return 0;
}

int mrh_dict_plan(void* h, int n, const uint8_t* buf, const int64_t* off, int nthreads, int64_t* units,
                  int64_t* tiles) {
  if (!h || !units || !tiles || bad_splits(n, buf, off)) return -1;
  Dict* d = static_cast<Dict*>(h);
  d->coded.assign((size_t)n, Coded());
  parallel(n, nthreads, [&](int, int i) {
    const int64_t len = off[i + 1] - off[i];
    if (len >= ((int64_t)1 << 32)) return;  // the tile index holds 32-bit positions
    encode_split(*d, buf + off[i], len, d->coded[(size_t)i]);
  });
  for (int i = 0; i < n; ++i) {
    const Coded& c = d->coded[(size_t)i];
    units[i] = c.done ? (int64_t)c.units.size() : -1;
    tiles[i] = c.done ? (int64_t)c.rows.size() / 2 - 1 : 0;
  }
  return 0;
}

int mrh_dict_run(void* h, int n, const int64_t* uoff, const int64_t* toff, uint8_t* out, uint32_t* tix,
                 int nthreads) {
  if (!h || !uoff || !toff || n < 0) return -1;
  Dict* d = static_cast<Dict*>(h);
  if ((size_t)n != d->coded.size()) return -1;
  for (int i = 0; i < n; ++i)
    if (uoff[i] >= 0 && (!d->coded[(size_t)i].done || !out || !tix || toff[i] < 0 || (uoff[i] & 1))) return -1;
  parallel(n, nthreads, [&](int, int i) {
    if (uoff[i] < 0) return;
    const Coded& c = d->coded[(size_t)i];
    if (!c.units.empty()) memcpy(out + uoff[i], c.units.data(), c.units.size() * 2);
    memcpy(tix + 2 * toff[i], c.rows.data(), c.rows.size() * 4);
  });
  std::vector<Coded>().swap(d->coded);
  return 0;
}

void mrh_dict_free(void* h) { delete static_cast<Dict*>(h); }

}  // extern "C"
