// pack_stress.cpp — sanitizer harness of the split packer (pack.cpp): seeded
// random splits over the alphabet sizes and lengths at which the packer takes
// another path, packed by several threads and checked against a
// byte-at-a-time decoder.  Built with pack.cpp under -fsanitize by
// tests/test_input_pack_sanitize.py; not part of libmrhost.so.
//
//   pack_stress [threads [rounds]]   -> prints "pack_stress ok", exit 0
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

extern "C" {
int64_t mrh_pack_plan(int n, const uint8_t* buf, const int64_t* off, int nthreads, int64_t* poff, int64_t* pbytes,
                      int32_t* k, uint8_t* tables);
int mrh_pack_run(int n, const uint8_t* buf, const int64_t* off, const int64_t* poff, const int32_t* k,
                 const uint8_t* tables, uint8_t* out, int nthreads);
}

namespace {

uint64_t rng_state = 0x9E3779B97F4A7C15ull;
uint64_t rnd() {
  rng_state ^= rng_state << 13;
  rng_state ^= rng_state >> 7;
  rng_state ^= rng_state << 17;
  return rng_state;
}

// symbol i of a packed split, read bit by bit
int symbol(const uint8_t* p, int k, int64_t i) {
  const int64_t bit0 = (i / 16) * 16 * k + (i % 16) * k;
  int c = 0;
  for (int b = 0; b < k; ++b) {
    const int64_t bit = bit0 + b;
    c |= ((p[bit >> 3] >> (bit & 7)) & 1) << b;
  }
  return c;
}

int fail(const char* what, int split) {
  fprintf(stderr, "pack_stress: %s (split %d)\n", what, split);
  return 1;
}

}  // namespace

int main(int argc, char** argv) {
  const int threads = argc > 1 ? atoi(argv[1]) : 8;
  const int rounds = argc > 2 ? atoi(argv[2]) : 2;
  const int alphabets[] = {1, 2, 3, 16, 17, 59, 64, 65, 128, 129, 256};
  const int64_t lengths[] = {1, 15, 16, 17, 31, 33, 4095, 4096, 4097, 70001};
  for (int round = 0; round < rounds; ++round) {
    std::vector<uint8_t> buf;
    std::vector<int64_t> off{0};
    std::vector<int> alpha;
    for (int a : alphabets)
      for (int64_t len : lengths) {
        // a random alphabet of a byte values; the first min(a, len) bytes show each once
        uint8_t perm[256];
        for (int i = 0; i < 256; ++i) perm[i] = (uint8_t)i;
        for (int i = 255; i > 0; --i) {
          const int j = (int)(rnd() % (uint64_t)(i + 1));
          const uint8_t t = perm[i];
          perm[i] = perm[j];
          perm[j] = t;
        }
        int used = 0;
        for (int64_t i = 0; i < len; ++i) {
          buf.push_back(i < a ? perm[i] : perm[rnd() % (uint64_t)a]);
          if (i < a) ++used;
        }
        off.push_back((int64_t)buf.size());
        alpha.push_back(used);
      }
    const int n = (int)off.size() - 1;
    std::vector<int64_t> poff(n), pbytes(n);
    std::vector<int32_t> k(n);
    std::vector<uint8_t> tables((size_t)n * 128);
    const int64_t total = mrh_pack_plan(n, buf.data(), off.data(), threads, poff.data(), pbytes.data(), k.data(),
                                        tables.data());
    if (total < 0) return fail("plan failed", -1);
    std::vector<uint8_t> out((size_t)total);  // exact size: an overrun is the sanitizer's to find
    if (mrh_pack_run(n, buf.data(), off.data(), poff.data(), k.data(), tables.data(), out.data(), threads) != 0)
      return fail("run failed", -1);
    int64_t at = 0;
    for (int i = 0; i < n; ++i) {
      const int64_t len = off[i + 1] - off[i];
      int want = 1;
      while ((1 << want) < alpha[i]) ++want;
      if (alpha[i] > 128) want = 8;
      if (k[i] != want) return fail("width is not the minimum", i);
      if (poff[i] % 16 != 0 || poff[i] != at) return fail("bad packed offset", i);
      if (pbytes[i] != (want == 8 ? 0 : (len + 15) / 16 * 2 * want)) return fail("bad packed size", i);
      at += (pbytes[i] + 15) / 16 * 16;
      if (want == 8) continue;
      const uint8_t* t = &tables[(size_t)i * 128];
      for (int c = 1; c < alpha[i]; ++c)
        if (t[c] <= t[c - 1]) return fail("table not ascending", i);
      for (int64_t j = 0; j < len; ++j)
        if (t[symbol(&out[poff[i]], want, j)] != buf[off[i] + j]) return fail("round trip differs", i);
      for (int64_t j = len; j < (len + 15) / 16 * 16; ++j)
        if (symbol(&out[poff[i]], want, j) != 0) return fail("padding is not zero", i);
    }
    if (at != total) return fail("bad total", -1);
  }
  printf("pack_stress ok\n");
  return 0;
}
