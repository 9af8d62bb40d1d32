// Number and token scanners of the text parsers, shared by the host runtime and the
// HIP text-parse kernels (csrc/hip/textparse.hip includes this file by relative path).
//
// Plain inline C++: no allocation, no library call except fma, every loop bounded by
// the token length, which is itself bounded by kMaxTok. A scanner returns
//   kOk    the value std::from_chars (csrc/core/data.cc to_u64 / to_i64 / to_f32)
//          gives for the same bytes, bit for bit;
//   kBad   bytes std::from_chars rejects (the line is a bad line);
//   kDefer the routine does not decide: the caller hands the text to the host parser.
// kBad is only reported when it is certain; anything doubtful is kDefer.
#pragma once
#include <math.h>
#include <stdint.h>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define TEXTNUM_HD __host__ __device__ inline
#else
#define TEXTNUM_HD inline
#endif

namespace textnum {

enum Status : int { kOk = 0, kBad = 1, kDefer = 2 };

// Longest token the scanners look at; a longer one is kDefer (the host decides).
constexpr int kMaxTok = 64;

TEXTNUM_HD uint64_t fmix(uint64_t k) {
  k ^= k >> 33;
  k *= 0xff51afd7ed558ccdull;
  k ^= k >> 33;
  k *= 0xc4ceb9fe1a85ec53ull;
  k ^= k >> 33;
  return k;
}

// Decimal u64: digits only (no sign, no blanks), overflow is an error.
TEXTNUM_HD int scan_u64(const uint8_t* p, int n, uint64_t* out) {
  if (n <= 0) return kBad;
  if (n > kMaxTok) return kDefer;
  uint64_t v = 0;
  for (int i = 0; i < n; ++i) {
    const unsigned d = (unsigned)p[i] - '0';
    if (d > 9) return kBad;
    if (v > 1844674407370955161ull || (v == 1844674407370955161ull && d > 5)) return kBad;
    v = v * 10 + d;
  }
  *out = v;
  return kOk;
}

// Decimal i64: one optional '+' (stripped by the caller's convention), then an optional
// '-', then digits; overflow is an error ("+-5" is -5, as the host parser has it).
TEXTNUM_HD int scan_i64(const uint8_t* p, int n, int64_t* out) {
  if (n > kMaxTok) return kDefer;
  int i = 0;
  if (i < n && p[i] == '+') ++i;
  bool neg = false;
  if (i < n && p[i] == '-') { neg = true; ++i; }
  if (i >= n) return kBad;
  const uint64_t lim = neg ? 9223372036854775808ull : 9223372036854775807ull;
  uint64_t v = 0;
  for (; i < n; ++i) {
    const unsigned d = (unsigned)p[i] - '0';
    if (d > 9) return kBad;
    if (v > (lim - d) / 10) return kBad;
    v = v * 10 + d;
  }
  *out = neg ? (int64_t)(0 - v) : (int64_t)v;
  return kOk;
}

// Hexadecimal u64: [0-9a-fA-F]+, no prefix, no sign; overflow is an error.
TEXTNUM_HD int scan_hex(const uint8_t* p, int n, uint64_t* out) {
  if (n <= 0) return kBad;
  if (n > kMaxTok) return kDefer;
  uint64_t v = 0;
  for (int i = 0; i < n; ++i) {
    const unsigned c = p[i];
    unsigned d;
    if (c - '0' <= 9u) d = c - '0';
    else if ((c | 0x20) - 'a' <= 5u) d = (c | 0x20) - 'a' + 10;
    else return kBad;
    if (v >> 60) return kBad;
    v = (v << 4) | d;
  }
  *out = v;
  return kOk;
}

// 10^e for 0 <= e <= 22: exactly representable doubles.
TEXTNUM_HD double pow10_exact(int e) {
  const double t[23] = {1e0,  1e1,  1e2,  1e3,  1e4,  1e5,  1e6,  1e7,  1e8,  1e9,  1e10, 1e11,
                        1e12, 1e13, 1e14, 1e15, 1e16, 1e17, 1e18, 1e19, 1e20, 1e21, 1e22};
  return t[e];
}

TEXTNUM_HD uint64_t f64_bits(double d) {
#if defined(__HIP_DEVICE_COMPILE__)
  return (uint64_t)__double_as_longlong(d);
#else
  union { double d; uint64_t u; } x;
  x.d = d;
  return x.u;
#endif
}

// f32 in std::from_chars "general" format after one optional '+': [-] digits [. digits]
// [(e|E) [+-] digits], at least one mantissa digit; an 'e' without exponent digits is a
// trailing-garbage error.
//
// Exact domain (else kDefer): at most 15 significant decimal digits m (trailing zeros not
// counted) and an effective
// decimal exponent |e| <= 22. m < 2^53 and 10^|e| are exact doubles, so d = m * 10^e or
// m / 10^-e is ONE correctly rounded operation, and |d| lies in [1e-22, 1e37], inside
// the normal float range. (float)d then equals the correctly rounded float of the
// decimal unless d is exactly half way between two floats while the decimal is not
// (monotone rounding keeps every other decimal on its side of every float midpoint):
// when the low 29 bits of d's significand are 1 followed by 28 zeros and the operation
// was inexact (fma residual != 0), the scanner defers. Zero mantissas give +-0.
TEXTNUM_HD int scan_f32(const uint8_t* p, int n, float* out) {
  if (n > kMaxTok) return kDefer;
  int i = 0;
  if (i < n && p[i] == '+') ++i;
  bool neg = false;
  if (i < n && p[i] == '-') { neg = true; ++i; }
  if (i >= n) return kBad;
  {
    const unsigned c = p[i] | 0x20;
    if (c == 'i' || c == 'n') return kDefer;  // inf / nan spellings
  }
  uint64_t m = 0;
  int nd = 0;        // significant digits taken into m
  bool dropped = false;  // a significant digit beyond the 15th (forces kDefer)
  int nfrac = 0;     // fraction digits taken into m
  int ndig = 0;      // mantissa digits seen at all
  int pz = 0, pz_frac = 0;  // zeros after the last non-zero digit (of them: in the fraction)
  bool dot = false;
  for (; i < n; ++i) {
    const unsigned c = p[i];
    const unsigned d = c - '0';
    if (d <= 9) {
      ++ndig;
      if (d == 0) {
        if (nd == 0) {  // leading zero
          if (dot) ++nfrac;
        } else {        // trailing so far: taken into m only when a digit follows
          ++pz;
          if (dot) ++pz_frac;
        }
        continue;
      }
      if (nd + pz + 1 > 15) {
        dropped = true;
        continue;
      }
      for (int z = 0; z < pz; ++z) m *= 10;
      m = m * 10 + d;
      nd += pz + 1;
      nfrac += pz_frac + (dot ? 1 : 0);
      pz = pz_frac = 0;
    } else if (c == '.' && !dot) {
      dot = true;
    } else {
      break;
    }
  }
  if (ndig == 0) return kBad;
  int ex = 0;
  bool ex_big = false;
  if (i < n) {
    if ((p[i] | 0x20) != 'e') return kBad;
    ++i;
    bool eneg = false;
    if (i < n && (p[i] == '+' || p[i] == '-')) { eneg = p[i] == '-'; ++i; }
    if (i >= n) return kBad;
    for (; i < n; ++i) {
      const unsigned d = (unsigned)p[i] - '0';
      if (d > 9) return kBad;
      if (ex < 100000) ex = ex * 10 + (int)d; else ex_big = true;
    }
    if (eneg) ex = -ex;
  }
  if (dropped || ex_big) return kDefer;
  if (m == 0) {
    *out = neg ? -0.0f : 0.0f;
    return kOk;
  }
  const int e10 = ex - nfrac + (pz - pz_frac);  // (integer trailing zeros scale up)
  if (e10 > 22 || e10 < -22) return kDefer;
  const double dm = (double)m;
  double d, resid;
  if (e10 >= 0) {
    const double pw = pow10_exact(e10);
    d = dm * pw;
    resid = fma(dm, pw, -d);
  } else {
    const double pw = pow10_exact(-e10);
    d = dm / pw;
    resid = fma(-d, pw, dm);
  }
  if ((f64_bits(d) & 0x1fffffffull) == 0x10000000ull && resid != 0.0) return kDefer;
  const float f = (float)d;
  *out = neg ? -f : f;
  return kOk;
}

// Criteo integer-slot bucket: v <= 0 ? 0 : floor(2 * log2(1 + v)) as the host computes it
// in double. floor(log2((1+v)^2)) = 63 - clz((1+v)^2) is that value for v < 2^31 (the
// square fits 64 bits; checked against the double expression, tests/test_textparse.py);
// larger v defer.
TEXTNUM_HD int criteo_bucket(int64_t v, uint64_t* id) {
  if (v <= 0) {
    *id = 0;
    return kOk;
  }
  if (v >= (int64_t)1 << 31) return kDefer;
  const uint64_t t = (uint64_t)v + 1;
  *id = (uint64_t)(63 - __builtin_clzll(t * t));
  return kOk;
}

}  // namespace textnum
