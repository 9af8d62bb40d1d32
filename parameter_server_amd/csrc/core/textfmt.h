// Number -> text for the key<TAB>weight model files, shared by the host runtime and the HIP
// model-text kernels (csrc/hip/modeltext.hip includes this file by relative path); the
// inverse direction of textnum.h.
//
// One entry is  str(key) + "\t" + format(float(w), ".9g") + "\n"  exactly as Python
// (utils/checkpoint.write_text_model) writes it. Plain inline C++: no allocation, no library
// call, no floating point -- '%.9g' is correctly rounded, and double arithmetic would round
// twice. An f32 is m * 2^e with m < 2^24; with X the decimal exponent of the rounded value
// and k = 8 - X its nine significant digits are N = round-half-even(m * 10^k * 2^e):
//   e >= 0  an exact left shift (e <= 6 below 2^30);
//   e <  0  (m * 10^k) >> -e with the shifted-out bits compared against half.
// m * 10^k is one 64 x 64 -> 128 bit product (10^k = 10^19 * 10^(k-19) for k > 19, the
// second factor folded into m), k <= 31 keeps it below 2^127, and no division wider than
// 32 bits occurs. X is not known up front: floor(log10 2^(e+23)) is X or X - 1, so the
// product is formed for that estimate and once more when it yields ten digits; a carry out
// of the rounding (N == 10^9) raises X by one.
//
// Exact domain: normal f32 with 1e-22 <= |w| < 1e9. Everything else (inf, nan, subnormals,
// larger, smaller) is kDefer and the caller formats the entry on the host; zero is kSkip
// (the writers drop zero and NaN weights before they get here; NaN is kDefer).
//
// A bare score, one column of a prediction file, is Python's "%.9g" % float(x) over the same
// domain plus the zeros the model writer never sees: +0 is "0" and -0 is "-0" (dec_score /
// put_score below).
#pragma once
#include "textnum.h"

namespace textfmt {

using textnum::kDefer;
using textnum::kOk;
constexpr int kSkip = 3;

constexpr int kMaxKey = 20;     // digits of 2^64 - 1
constexpr int kMaxWeight = 15;  // "-d.dddddddde-XX", "-0.000ddddddddd"
constexpr int kMaxEntry = kMaxKey + 1 + kMaxWeight + 1;

// A weight ready to be written: nine digits, how many of them are significant once the
// trailing zeros are dropped, the decimal exponent, the sign and the text length.
struct Dec {
  uint32_t n9;  // 10^8 <= n9 < 10^9
  int nd;       // 1..9
  int x;        // -22..8
  bool neg;
};

TEXTNUM_HD uint64_t pow10_u64(int e) {  // 0 <= e <= 19
  const uint64_t t[20] = {1ull,
                          10ull,
                          100ull,
                          1000ull,
                          10000ull,
                          100000ull,
                          1000000ull,
                          10000000ull,
                          100000000ull,
                          1000000000ull,
                          10000000000ull,
                          100000000000ull,
                          1000000000000ull,
                          10000000000000ull,
                          100000000000000ull,
                          1000000000000000ull,
                          10000000000000000ull,
                          100000000000000000ull,
                          1000000000000000000ull,
                          10000000000000000000ull};
  return t[e];
}

// floor(m * 10^k * 2^e) and whether round-half-even goes up. 0 <= k <= 31, -127 <= e <= 6,
// m < 2^24, and the caller's choice of k keeps the result below 10^10.
TEXTNUM_HD uint64_t scaled(uint32_t m, int e, int k, bool* up) {
  const uint64_t a = k > 19 ? (uint64_t)m * pow10_u64(k - 19) : (uint64_t)m;
  const uint64_t b = pow10_u64(k > 19 ? 19 : k);
  const unsigned __int128 p = (unsigned __int128)a * b;
  if (e >= 0) {
    *up = false;
    return (uint64_t)(p << e);
  }
  const int s = -e;
  const unsigned __int128 q = p >> s;
  const unsigned __int128 rem = p - (q << s), half = (unsigned __int128)1 << (s - 1);
  *up = rem > half || (rem == half && ((uint64_t)q & 1u));
  return (uint64_t)q;
}

// kOk: *d describes the weight with these bits; kSkip: +-0; kDefer: outside the domain.
TEXTNUM_HD int dec_f32(uint32_t bits, Dec* d) {
  const int be = (int)((bits >> 23) & 0xffu);
  const uint32_t frac = bits & 0x7fffffu;
  if (be == 0 && frac == 0) return kSkip;
  if (be == 0 || be == 255) return kDefer;  // subnormal, inf, nan
  const uint32_t m = frac | 0x800000u;
  const int e = be - 150;       // |w| = m * 2^e, 2^(e+23) <= |w| < 2^(e+24)
  if (e > 6 || e < -97) return kDefer;  // |w| >= 2^30 > 1e9, |w| < 2^-74 < 1e-22
  // floor((e + 23) * log10(2)): 78913 / 2^18 is log10(2) to 8 digits, exact floor for |t| < 1000
  int x = ((e + 23) * 78913) >> 18;
  bool up;
  uint64_t q = scaled(m, e, 8 - x, &up);
  if (q >= 1000000000ull) {  // ten digits: the estimate was one low
    ++x;
    if (x > 8) return kDefer;  // |w| >= 1e9
    q = scaled(m, e, 8 - x, &up);
  }
  if (up) ++q;
  if (q >= 1000000000ull) {  // the rounding carried into the next power of ten
    q = 100000000ull;
    ++x;
  }
  if (x > 8 || x < -22) return kDefer;
  uint32_t n9 = (uint32_t)q;
  int nd = 9;
  d->n9 = n9;
  while (nd > 1 && n9 % 10u == 0) {
    n9 /= 10u;
    --nd;
  }
  d->nd = nd;
  d->x = x;
  d->neg = (bits >> 31) != 0;
  return kOk;
}

TEXTNUM_HD int weight_len(const Dec& d) {
  const int s = d.neg ? 1 : 0;
  if (d.x >= 0) return s + d.x + 1 + (d.nd > d.x + 1 ? d.nd - d.x : 0);  // ddd[.ddd]
  if (d.x >= -4) return s + 1 - d.x + d.nd;                              // 0.00ddd
  return s + d.nd + (d.nd > 1 ? 1 : 0) + 4;                              // d[.ddd]e-XX
}

// Writes weight_len(d) bytes.
template <typename Out>
TEXTNUM_HD int put_weight(const Dec& d, Out* out) {
  uint8_t dig[9];
  uint32_t v = d.n9;
#pragma unroll
  for (int i = 8; i >= 0; --i) {
    dig[i] = (uint8_t)('0' + v % 10u);
    v /= 10u;
  }
  int o = 0;
  if (d.neg) out[o++] = '-';
  if (d.x >= 0) {
    const int ni = d.x + 1;  // integer digits (<= 9: the zeros among them are in dig)
#pragma unroll
    for (int i = 0; i < 9; ++i) {
      if (i == ni && i < d.nd) out[o++] = '.';
      if (i < ni || i < d.nd) out[o++] = dig[i];
    }
  } else if (d.x >= -4) {
    out[o++] = '0';
    out[o++] = '.';
    for (int z = -1; z > d.x; --z) out[o++] = '0';
#pragma unroll
    for (int i = 0; i < 9; ++i)
      if (i < d.nd) out[o++] = dig[i];
  } else {
    out[o++] = dig[0];
    if (d.nd > 1) out[o++] = '.';
#pragma unroll
    for (int i = 1; i < 9; ++i)
      if (i < d.nd) out[o++] = dig[i];
    const int ax = -d.x;  // 5..22
    out[o++] = 'e';
    out[o++] = '-';
    out[o++] = (uint8_t)('0' + ax / 10);
    out[o++] = (uint8_t)('0' + ax % 10);
  }
  return o;
}

// A score column: dec_f32 with +-0 inside the domain. A zero is the Dec {n9 = 0, nd = 1,
// x = 0}, which weight_len / put_weight already turn into "0" / "-0" (one integer digit, no
// fraction), so the callers need no second case. kOk or kDefer, never kSkip.
constexpr int kMaxScore = kMaxWeight;

TEXTNUM_HD int dec_score(uint32_t bits, Dec* d) {
  if ((bits & 0x7fffffffu) == 0) {
    d->n9 = 0;
    d->nd = 1;
    d->x = 0;
    d->neg = (bits >> 31) != 0;
    return kOk;
  }
  return dec_f32(bits, d);
}

// The score with these bits into out (room for kMaxScore bytes, no terminator). kOk: *len
// bytes written; kDefer: nothing written, *len = 0.
TEXTNUM_HD int put_score(uint32_t bits, uint8_t* out, int* len) {
  Dec d;
  *len = 0;
  const int st = dec_score(bits, &d);
  if (st != kOk) return st;
  *len = put_weight(d, out);
  return kOk;
}

TEXTNUM_HD int key_len(uint64_t k) {
  int n = 1;
  while (k >= 10u) {
    k /= 10u;
    ++n;
  }
  return n;
}

// Writes the len = key_len(k) digits of k.
template <typename Out>
TEXTNUM_HD void put_key(uint64_t k, int len, Out* out) {
  for (int i = len - 1; i >= 0; --i) {
    out[i] = (uint8_t)('0' + (unsigned)(k % 10u));
    k /= 10u;
  }
}

// One whole entry into out (room for kMaxEntry bytes). kOk: *len bytes written; kSkip
// (zero weight) / kDefer: nothing written, *len = 0.
TEXTNUM_HD int put_entry(uint64_t key, uint32_t wbits, uint8_t* out, int* len) {
  Dec d;
  *len = 0;
  const int st = dec_f32(wbits, &d);
  if (st != kOk) return st;
  const int kl = key_len(key);
  put_key(key, kl, out);
  out[kl] = '\t';
  const int wl = put_weight(d, out + kl + 1);
  out[kl + 1 + wl] = '\n';
  *len = kl + wl + 2;
  return kOk;
}

}  // namespace textfmt
