// Stand-alone fuzz driver of the bare-score formatter the prediction writer's kernels share
// with the host (csrc/core/textfmt.h dec_score / put_score), meant to be built with
// -fsanitize=address,undefined: boundary and seeded random f32 bit patterns, each formatted
// into a heap block of exactly the length the formatter announces (and once into one of
// exactly kMaxScore bytes), so that a write past the score is an AddressSanitizer error.
// Where the formatter reports text it is compared with snprintf("%.9g") of the same value,
// which is correctly rounded as Python's format is; +-0 must be "0" / "-0" and inside the
// domain, everything dec_f32 defers must still defer.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>

#include "textfmt.h"

static uint64_t rng_state = 0x2545f4914f6cdd1dull;
static uint64_t rnd() {
  uint64_t z = (rng_state += 0x9e3779b97f4a7c15ull);
  z = (z ^ (z >> 30)) * 0xbf58476d1ce4e5b9ull;
  z = (z ^ (z >> 27)) * 0x94d049bb133111ebull;
  return z ^ (z >> 31);
}

static long failures = 0, formatted = 0, zeros = 0;

static void fail(const char* what, uint32_t bits, const std::string& got, const std::string& want) {
  ++failures;
  std::fprintf(stderr, "FAIL %s bits=0x%08x got=\"%s\" want=\"%s\"\n", what, bits, got.c_str(),
               want.c_str());
}

static void check(uint32_t bits) {
  float x;
  std::memcpy(&x, &bits, 4);
  const double a = std::fabs((double)x);
  const bool zero = (bits & 0x7fffffffu) == 0;
  const bool in_domain =
      zero || (std::isfinite(x) && a >= 1e-22 && a < 1e9 && (bits & 0x7f800000u) != 0);

  uint8_t* full = (uint8_t*)std::malloc(textfmt::kMaxScore);
  int len = -1;
  const int st = textfmt::put_score(bits, full, &len);
  if (st != textnum::kOk) {
    if (st != textnum::kDefer) fail("status is neither kOk nor kDefer", bits, "", "");
    if (len != 0) fail("length of an unwritten score", bits, "", "");
    if (in_domain) fail("in-domain value not formatted", bits, "", "");
    std::free(full);
    return;
  }
  ++formatted;
  zeros += zero;
  char ref[64];
  const int rl = std::snprintf(ref, sizeof ref, "%.9g", (double)x);
  const std::string want(ref, (size_t)rl), got((const char*)full, (size_t)len);
  std::free(full);
  if (!in_domain) fail("out-of-domain value formatted", bits, got, want);
  if (got != want) fail("text differs", bits, got, want);
  if (zero && got != (bits ? "-0" : "0")) fail("zero", bits, got, want);

  // the pieces the kernels call, into a block of exactly the announced length
  textfmt::Dec d;
  if (textfmt::dec_score(bits, &d) != textnum::kOk) {
    fail("dec_score disagrees with put_score", bits, got, want);
    return;
  }
  const int wl = textfmt::weight_len(d);
  if (wl != len || wl < 1 || wl > textfmt::kMaxScore) fail("announced length", bits, got, want);
  uint8_t* wb = (uint8_t*)std::malloc((size_t)wl);
  if (textfmt::put_weight(d, wb) != wl) fail("put_weight length", bits, got, want);
  if (std::memcmp(wb, got.data(), (size_t)(wl < len ? wl : len)) != 0)
    fail("pieces differ from the score", bits, got, want);
  std::free(wb);
  // dec_score is dec_f32 except at the zeros
  textfmt::Dec d2;
  const int s2 = textfmt::dec_f32(bits, &d2);
  if (zero ? s2 != textfmt::kSkip : s2 != textnum::kOk) fail("dec_f32 status", bits, got, want);
}

static uint32_t bits_of(float f) {
  uint32_t b;
  std::memcpy(&b, &f, 4);
  return b;
}

int main() {
  check(0u);
  check(0x80000000u);
  // every binade, smallest / largest / a middle mantissa, both signs; subnormals, inf, nan
  for (uint32_t be = 0; be < 256; ++be)
    for (uint32_t fr : {0u, 1u, 0x400000u, 0x7ffffeu, 0x7fffffu})
      for (uint32_t s : {0u, 0x80000000u}) check(s | (be << 23) | fr);
  // powers of ten and their float neighbours, the ties, the notation switches
  for (int e = -30; e <= 12; ++e) {
    const uint32_t b = bits_of((float)std::pow(10.0, e));
    for (int dlt = -2; dlt <= 2; ++dlt) {
      check(b + (uint32_t)dlt);
      check((b + (uint32_t)dlt) | 0x80000000u);
    }
  }
  for (float f : {1000000.125f, 1000000.375f, 999999999.0f, 999999936.0f, 999999.9375f, 0.0001f,
                  0.000099999997f, 3e9f, 1e-30f, 0.5f, 1.0f, 123456792.0f, 0.1f,
                  0.000123456784f, 1.23456787e-22f})
    for (uint32_t s : {0u, 0x80000000u}) check(bits_of(f) | s);
  // random bit patterns (all of f32)
  for (int i = 0; i < 1000000; ++i) check((uint32_t)rnd());
  // random patterns confined to the domain's binades
  for (int i = 0; i < 500000; ++i) {
    const uint64_t r = rnd();
    const uint32_t be = 53 + (uint32_t)((r >> 40) % 104);  // 2^-74 .. 2^29
    check(((uint32_t)r & 0x807fffffu) | (be << 23));
  }
  if (failures || zeros < 2) {
    std::fprintf(stderr, "scorefmt_fuzz: %ld failures, %ld zeros formatted\n", failures, zeros);
    return 1;
  }
  std::printf("scorefmt_fuzz OK (%ld scores formatted)\n", formatted);
  return 0;
}
