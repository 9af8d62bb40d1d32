// Stand-alone fuzz driver of the model-text formatter the GPU writer shares with the host
// (csrc/core/textfmt.h), meant to be built with -fsanitize=address,undefined: boundary and
// seeded random (key, f32) pairs, each formatted into a heap block of exactly the length
// the formatter announces (and once into one of exactly kMaxEntry bytes), so that a write
// past the entry is an AddressSanitizer error. Where the formatter reports text, the
// weight is compared with snprintf("%.9g") of the same value, which is correctly rounded
// as Python's format is.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>

#include "textfmt.h"

static uint64_t rng_state = 0x9e3779b97f4a7c15ull;
static uint64_t rnd() {
  uint64_t z = (rng_state += 0x9e3779b97f4a7c15ull);
  z = (z ^ (z >> 30)) * 0xbf58476d1ce4e5b9ull;
  z = (z ^ (z >> 27)) * 0x94d049bb133111ebull;
  return z ^ (z >> 31);
}

static long failures = 0, formatted = 0;

static void fail(const char* what, uint64_t key, uint32_t bits, const std::string& got,
                 const std::string& want) {
  ++failures;
  std::fprintf(stderr, "FAIL %s key=%llu bits=0x%08x got=\"%s\" want=\"%s\"\n", what,
               (unsigned long long)key, bits, got.c_str(), want.c_str());
}

static void check(uint64_t key, uint32_t bits) {
  float w;
  std::memcpy(&w, &bits, 4);
  const double a = std::fabs((double)w);
  const bool in_domain = std::isfinite(w) && a >= 1e-22 && a < 1e9 && (bits & 0x7f800000u) != 0;

  uint8_t* full = (uint8_t*)std::malloc(textfmt::kMaxEntry);
  int len = -1;
  const int st = textfmt::put_entry(key, bits, full, &len);
  if (st != textnum::kOk) {
    if (len != 0) fail("length of an unwritten entry", key, bits, "", "");
    if (in_domain) fail("in-domain value not formatted", key, bits, "", "");
    if (st == textfmt::kSkip && w != 0.0f) fail("non-zero skipped", key, bits, "", "");
    std::free(full);
    return;
  }
  ++formatted;
  char ref[64];
  const int rl = std::snprintf(ref, sizeof ref, "%llu\t%.9g\n", (unsigned long long)key, (double)w);
  const std::string want(ref, (size_t)rl), got((const char*)full, (size_t)len);
  if (!in_domain) fail("out-of-domain value formatted", key, bits, got, want);
  if (got != want) fail("text differs", key, bits, got, want);
  std::free(full);

  // the pieces, each into a block of exactly its announced length
  textfmt::Dec d;
  if (textfmt::dec_f32(bits, &d) != textnum::kOk) {
    fail("dec_f32 disagrees with put_entry", key, bits, got, want);
    return;
  }
  const int wl = textfmt::weight_len(d), kl = textfmt::key_len(key);
  if (kl + wl + 2 != len || kl > textfmt::kMaxKey || wl > textfmt::kMaxWeight)
    fail("announced lengths", key, bits, got, want);
  uint8_t* wb = (uint8_t*)std::malloc((size_t)wl);
  if (textfmt::put_weight(d, wb) != wl) fail("put_weight length", key, bits, got, want);
  uint8_t* kb = (uint8_t*)std::malloc((size_t)kl);
  textfmt::put_key(key, kl, kb);
  if (std::memcmp(kb, got.data(), (size_t)kl) != 0 ||
      std::memcmp(wb, got.data() + kl + 1, (size_t)wl) != 0)
    fail("pieces differ from the entry", key, bits, got, want);
  std::free(wb);
  std::free(kb);
}

static uint32_t bits_of(float f) {
  uint32_t b;
  std::memcpy(&b, &f, 4);
  return b;
}

int main() {
  const uint64_t keys[] = {0ull, 9ull, 10ull, 1ull << 32, (1ull << 63) - 1, 1ull << 63, ~0ull,
                           9999999999999999999ull, 10000000000000000000ull};
  const int nkeys = (int)(sizeof keys / sizeof keys[0]);
  int ki = 0;
  // every binade, smallest / largest / a middle mantissa, both signs; zero, subnormals, inf, nan
  for (uint32_t be = 0; be < 256; ++be)
    for (uint32_t fr : {0u, 1u, 0x400000u, 0x7ffffeu, 0x7fffffu})
      for (uint32_t s : {0u, 0x80000000u}) check(keys[ki++ % nkeys], s | (be << 23) | fr);
  // powers of ten and their float neighbours, the ties, the notation switches
  for (int e = -30; e <= 12; ++e) {
    const uint32_t b = bits_of((float)std::pow(10.0, e));
    for (int dlt = -2; dlt <= 2; ++dlt) {
      check(keys[ki++ % nkeys], b + (uint32_t)dlt);
      check(keys[ki++ % nkeys], (b + (uint32_t)dlt) | 0x80000000u);
    }
  }
  for (float f : {1000000.125f, 1000000.375f, 999999999.0f, 999999936.0f, 0.0001f, 0.000099999997f,
                  3e9f, 1e-30f, 0.5f, 1.0f, 123456792.0f, 0.1f})
    for (uint32_t s : {0u, 0x80000000u}) check(keys[ki++ % nkeys], bits_of(f) | s);
  // random bit patterns (all of f32), random keys of every length
  for (int i = 0; i < 1000000; ++i) {
    const uint64_t r = rnd();
    uint64_t key = rnd();
    key >>= (r >> 32) % 64;
    check(key, (uint32_t)r);
  }
  // random patterns confined to the domain's binades
  for (int i = 0; i < 500000; ++i) {
    const uint64_t r = rnd();
    const uint32_t be = 53 + (uint32_t)((r >> 40) % 104);  // 2^-74 .. 2^29
    check(rnd() >> (r % 64), ((uint32_t)r & 0x807fffffu) | (be << 23));
  }
  if (failures) {
    std::fprintf(stderr, "textfmt_fuzz: %ld failures\n", failures);
    return 1;
  }
  std::printf("textfmt_fuzz OK (%ld entries formatted)\n", formatted);
  return 0;
}
