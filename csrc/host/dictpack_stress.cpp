// dictpack_stress.cpp — sanitizer harness of the dictionary packer
// (dictpack.cpp): seeded random splits (word text over small and large
// vocabularies, no whitespace at all, whitespace only, every byte value, tokens
// of 31 and 32 bytes, empty splits), coded by several threads into buffers of
// exactly the planned size and checked with a byte-at-a-time decoder.  Built
// with dictpack.cpp under -fsanitize by tests/test_input_dict_sanitize.py; not
// part of libmrhost.so.
//
//   dictpack_stress [threads [rounds]]   -> prints "dictpack_stress ok", exit 0
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

extern "C" {
void* mrh_dict_build(int n, const uint8_t* buf, const int64_t* off, int nthreads, int64_t max_entries);
int64_t mrh_dict_entries(void* h);
int mrh_dict_slots(void* h, uint8_t* out);
int mrh_dict_plan(void* h, int n, const uint8_t* buf, const int64_t* off, int nthreads, int64_t* units, int64_t* tiles);
int mrh_dict_run(void* h, int n, const int64_t* uoff, const int64_t* toff, uint8_t* out, uint32_t* tix, int nthreads);
void mrh_dict_free(void* h);
}

namespace {

uint64_t rng_state = 0x9E3779B97F4A7C15ull;
uint64_t rnd() {
  rng_state ^= rng_state << 13;
  rng_state ^= rng_state >> 7;
  rng_state ^= rng_state << 17;
  return rng_state;
}

int fail(const char* what, int split) {
  fprintf(stderr, "dictpack_stress: %s (split %d)\n", what, split);
  return 1;
}

void words(std::vector<uint8_t>& buf, int64_t len, int vocab, int maxlen) {
  const char seps[] = " \t\n\v\f\r";
  const int64_t end = (int64_t)buf.size() + len;
  while ((int64_t)buf.size() < end) {
    const uint64_t w = rnd() % (uint64_t)vocab;
    const int wl = 1 + (int)(w % (uint64_t)maxlen);
    std::string s = std::to_string(w * 2654435761ull);
    while ((int)s.size() < wl) s += s;
    s.resize((size_t)wl);
    for (char c : s)
      if ((int64_t)buf.size() < end) buf.push_back((uint8_t)c);
    if ((int64_t)buf.size() < end) buf.push_back((uint8_t)seps[rnd() % 8 < 6 ? 0 : rnd() % 6]);
  }
}

}  // namespace

int main(int argc, char** argv) {
  const int threads = argc > 1 ? atoi(argv[1]) : 8;
  const int rounds = argc > 2 ? atoi(argv[2]) : 2;
  const int64_t lengths[] = {0, 1, 2, 15, 16, 17, 31, 32, 33, 4095, 4097, 8193, 70001};
  for (int round = 0; round < rounds; ++round) {
    std::vector<uint8_t> buf;
    std::vector<int64_t> off{0};
    for (int kind = 0; kind < 6; ++kind)
      for (int64_t len : lengths) {
        const int64_t end = (int64_t)buf.size() + len;
        if (kind == 0) words(buf, len, 40, 8);
        if (kind == 1) words(buf, len, 70000, 40);  // two-unit codes, tokens longer than 31 bytes
        if (kind == 2)
          while ((int64_t)buf.size() < end) buf.push_back((uint8_t)(33 + rnd() % 94));  // no whitespace
        if (kind == 3)
          while ((int64_t)buf.size() < end) buf.push_back((uint8_t)" \t\n\v\f\r"[rnd() % 6]);
        if (kind == 4)
          while ((int64_t)buf.size() < end) buf.push_back((uint8_t)rnd());
        if (kind == 5)
          while ((int64_t)buf.size() < end) buf.push_back((uint8_t)((buf.size() % 63) < 31 ? 'x' : (buf.size() % 63) == 31 ? ' ' : (buf.size() % 63) == 62 ? '\n' : 'y'));
        off.push_back((int64_t)buf.size());
      }
    const int n = (int)off.size() - 1;
    const int64_t cap = round == 0 ? (1 << 20) : 300 + round;
    void* h = mrh_dict_build(n, buf.data(), off.data(), threads, cap);
    if (!h) return fail("build failed", -1);
    const int64_t entries = mrh_dict_entries(h);
    if (entries < 256 || entries > cap) return fail("bad entry count", -1);
    std::vector<uint8_t> slots((size_t)entries * 32);  // exact size: an overrun is the sanitizer's to find
    if (mrh_dict_slots(h, slots.data()) != 0) return fail("slots failed", -1);
    std::vector<int64_t> units(n), tiles(n), uoff(n), toff(n);
    if (mrh_dict_plan(h, n, buf.data(), off.data(), threads, units.data(), tiles.data()) != 0)
      return fail("plan failed", -1);
    int64_t ub = 0, rows = 0;
    for (int i = 0; i < n; ++i) {
      if (units[i] < 0) return fail("split not coded", i);
      const bool skip = i % 7 == 3;  // some splits stay in another form
      uoff[i] = skip ? -1 : ub;
      toff[i] = rows;
      if (!skip) {
        ub += units[i] * 2;
        rows += tiles[i] + 1;
      }
    }
    std::vector<uint8_t> out((size_t)ub);
    std::vector<uint32_t> tix((size_t)rows * 2);
    if (mrh_dict_run(h, n, uoff.data(), toff.data(), out.data(), tix.data(), threads) != 0)
      return fail("run failed", -1);
    mrh_dict_free(h);
    for (int i = 0; i < n; ++i) {
      if (uoff[i] < 0) continue;
      const int64_t len = off[i + 1] - off[i];
      const uint32_t* row = &tix[(size_t)toff[i] * 2];
      int64_t at = 0, tile = 0;
      for (int64_t u = 0; u < units[i];) {
        uint16_t a, b = 0;
        memcpy(&a, &out[(size_t)(uoff[i] + 2 * u)], 2);
        int64_t e = a, nu = 1;
        if (a >= 0xC000) {
          if (u + 1 >= units[i]) return fail("a lead is the last unit", i);
          memcpy(&b, &out[(size_t)(uoff[i] + 2 * u + 2)], 2);
          if (b >= 0xC000) return fail("a lead follows a lead", i);
          e = 0xC000 + (int64_t)(a - 0xC000) * 0xC000 + b;
          nu = 2;
        }
        if (e >= entries) return fail("entry beyond the dictionary", i);
        const uint8_t* s = &slots[(size_t)e * 32];
        const int l = s[31];
        if (l < 1 || l > 31 || at + l > len || memcmp(s, &buf[(size_t)(off[i] + at)], (size_t)l) != 0)
          return fail("round trip differs", i);
        if (tile < tiles[i] && row[2 * tile] == (uint32_t)u) {
          if (row[2 * tile + 1] != (uint32_t)at) return fail("tile starts at the wrong byte", i);
          ++tile;
        }
        if (tile == 0 || u + nu - row[2 * (tile - 1)] > 4096 || at + l - row[2 * (tile - 1) + 1] > 8192)
          return fail("tile over its limits", i);
        u += nu;
        at += l;
      }
      if (at != len) return fail("decoded length differs", i);
      if (tile != tiles[i] || row[2 * tiles[i]] != (uint32_t)units[i] || row[2 * tiles[i] + 1] != (uint32_t)len)
        return fail("bad tile index", i);
    }
  }
  printf("dictpack_stress ok\n");
  return 0;
}
