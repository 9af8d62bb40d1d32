// Stand-alone fuzz driver of the scanners the GPU text parser shares with the host
// (csrc/core/textnum.h), meant to be built with -fsanitize=address,undefined: seeded
// random byte strings and the boundary strings, each copied into an exactly sized heap
// block so that a read past the token is an AddressSanitizer error. Where a scanner
// reports a value it is compared with std::from_chars, which the host parser uses.
#include <charconv>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "textnum.h"

static uint64_t rng_state = 0x9e3779b97f4a7c15ull;
static uint64_t rnd() {
  uint64_t z = (rng_state += 0x9e3779b97f4a7c15ull);
  z = (z ^ (z >> 30)) * 0xbf58476d1ce4e5b9ull;
  z = (z ^ (z >> 27)) * 0x94d049bb133111ebull;
  return z ^ (z >> 31);
}

static long failures = 0;
#define EXPECT(cond, s)                                                         \
  do {                                                                          \
    if (!(cond)) {                                                              \
      ++failures;                                                               \
      std::fprintf(stderr, "FAIL %s on \"%s\" (line %d)\n", #cond, (s).c_str(), __LINE__); \
    }                                                                           \
  } while (0)

template <typename T, typename... Base>
static bool ref_parse(const char* b, const char* e, T* v, Base... base) {
  auto r = std::from_chars(b, e, *v, base...);
  return r.ec == std::errc() && r.ptr == e;
}

static void check(const std::string& s) {
  // exactly sized copy: one byte past the token is out of bounds
  uint8_t* p = (uint8_t*)std::malloc(s.size() ? s.size() : 1);
  std::memcpy(p, s.data(), s.size());
  const int n = (int)s.size();
  const char* b = (const char*)p;
  const char* e = b + n;
  const bool too_long = n > textnum::kMaxTok;
  {
    uint64_t v = 0, r = 0;
    const int st = textnum::scan_u64(p, n, &v);
    const bool ok = ref_parse(b, e, &r);
    if (too_long) EXPECT(st == textnum::kDefer, s);
    else EXPECT(st == (ok ? textnum::kOk : textnum::kBad), s);
    if (st == textnum::kOk) EXPECT(v == r, s);
  }
  {
    int64_t v = 0, r = 0;
    const int st = textnum::scan_i64(p, n, &v);
    const bool ok = ref_parse(b + (n > 0 && *b == '+'), e, &r);
    if (too_long) EXPECT(st == textnum::kDefer, s);
    else EXPECT(st == (ok ? textnum::kOk : textnum::kBad), s);
    if (st == textnum::kOk) EXPECT(v == r, s);
  }
  {
    uint64_t v = 0, r = 0;
    const int st = textnum::scan_hex(p, n, &v);
    const bool ok = ref_parse(b, e, &r, 16);
    if (too_long) EXPECT(st == textnum::kDefer, s);
    else EXPECT(st == (ok ? textnum::kOk : textnum::kBad), s);
    if (st == textnum::kOk) EXPECT(v == r, s);
  }
  {
    float v = 0, r = 0;
    const int st = textnum::scan_f32(p, n, &v);
    const bool ok = ref_parse(b + (n > 0 && *b == '+'), e, &r);
    if (st == textnum::kOk) {
      EXPECT(ok, s);
      EXPECT(std::memcmp(&v, &r, 4) == 0, s);
    } else if (st == textnum::kBad) {
      EXPECT(!ok, s);
    }
  }
  std::free(p);
}

int main() {
  const char* hand[] = {"", "+", "-", ".", "e", "E", "+.", "-.", ".e1", "1e", "1e+", "1e-", "--1",
                        "+-1", "-+1", "++1", "1.2.3", "0", "-0", "+0", "00", "1", "0.1", ".5", "5.",
                        "16777217", "1e-45", "3.4028235e38", "3.4028236e38", "1e39", "1e-39",
                        "inf", "nan", "-inf", "INF", "NaN", "infinity", "nan(1)", "0x10", "1f",
                        "12345678901234567890", "18446744073709551615", "18446744073709551616",
                        "99999999999999999999", "9223372036854775807", "9223372036854775808",
                        "-9223372036854775808", "-9223372036854775809", "ffffffffffffffff",
                        "10000000000000000", "FFFFFFFFFFFFFFFFF", "1e22", "1e23", "1e-22",
                        "1e-23", "123456789012345e22", "1234567890123456", "0.000000000000001",
                        "1e99999999999", "0e99999999999", "1e-99999999999", "100000000000000000000",
                        "0.30000000000000004", "9007199254740993", "1 ", " 1", "1\t", "1:1"};
  for (const char* h : hand) check(h);
  for (int len : {63, 64, 65, 66, 200}) {  // the token-length bound
    check(std::string(len, '0'));
    check(std::string(len, '9'));
    check(std::string(len, 'f'));
    check("0." + std::string(len - 2, '3'));
    check(std::string(len - 1, '0') + "1");
    check("1e" + std::string(len - 2, '0'));
    check("-" + std::string(len - 1, '7'));
  }
  const std::string digits = "0123456789", numeric = "0123456789+-.eE", hexd = "0123456789abcdefABCDEFxX";
  for (int it = 0; it < 400000; ++it) {
    const int len = (int)(rnd() % 24);
    std::string s(len, '\0');
    const int kind = (int)(rnd() % 4);
    for (int i = 0; i < len; ++i) {
      const uint64_t r = rnd();
      s[i] = kind == 0 ? (char)(r & 0xff)
           : kind == 1 ? digits[r % digits.size()]
           : kind == 2 ? numeric[r % numeric.size()]
                       : hexd[r % hexd.size()];
    }
    check(s);
  }
  for (int it = 0; it < 200000; ++it) {  // well-formed decimals, many digits and exponents
    std::string s;
    if (rnd() % 3 == 0) s += "+-"[rnd() % 2];
    const int ni = (int)(rnd() % 20), nf = (int)(rnd() % 20);
    for (int i = 0; i < ni; ++i) s += digits[rnd() % 10];
    if (rnd() % 2) {
      s += '.';
      for (int i = 0; i < nf; ++i) s += digits[rnd() % 10];
    }
    if (rnd() % 2) s += "eE"[rnd() % 2] + std::string(rnd() % 2 ? "-" : "") + std::to_string(rnd() % 45);
    check(s);
  }
  uint64_t id = 0;
  const int64_t vs[] = {INT64_MIN, -1, 0, 1, 2, 3, (1ll << 31) - 2, (1ll << 31) - 1, 1ll << 31,
                        INT64_MAX};
  for (int64_t v : vs) {
    const int st = textnum::criteo_bucket(v, &id);
    if (v >= (1ll << 31)) {
      if (st != textnum::kDefer) ++failures;
    } else if (st != textnum::kOk) {
      ++failures;
    }
  }
  (void)textnum::fmix(0x0123456789abcdefull);
  if (failures) {
    std::fprintf(stderr, "textnum_fuzz: %ld failures\n", failures);
    return 1;
  }
  std::puts("textnum_fuzz OK");
  return 0;
}
