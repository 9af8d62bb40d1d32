// ADFEA ("lineid 1 click key:grp key:grp ...") and TERAFEA ("click lineid | key key ...")
// text -> CSR minibatch arrays and per-feature slot ids on the device (gfx950), the device
// half of csrc/core/data.cc parse_adfea / parse_terafea with parse_range. A third strict
// fast path next to textparse.hip and pstext.hip, with the same decomposition
// (textparse.cuh): 16 KiB of text per 1024-thread workgroup, count -> scan -> emit -> finish
// in separate launches, no hand-off between workgroups, no global atomics on the data.
//
// Token bytes are everything except '\n', blank, tab, CR and (ADFEA) ':'; a token belongs to
// the thread that holds its first byte. What a token is depends on its index t within its
// line only:
//   ADFEA    t < 2 skipped, t == 2 the label, odd t >= 3 a key, even t >= 4 that key's group
//            (the token that makes the entry);
//   TERAFEA  t == 0 the label, t == 1, 2 skipped, t >= 3 a key (one entry each).
// One carry decides t, "tokens since the last '\n'", a function of the carry-in that composes
// associatively (TokFn): text with a newline resets it to its tail count, text without one
// adds its token count. Labels and entry tokens among the line indices [0, x) have closed
// forms (labs_below, ents_below), so:
//   1. ad_count   per span: its TokFn, h = the tokens before its first '\n' (their classes
//                 depend on the carry) and the labels / entry tokens of the lines that start
//                 inside it (they do not).
//   2. ad_scan    one workgroup: scans the carry, books each span's head segment in closed
//                 form from (carry_in, h), scans labels and entries, header, capacity check.
//   3. ad_emit    re-classifies with the true carry; one thread per token parses it. The
//                 label writes labels[R] and row_ptr[R]; a key writes keys[E], E the entry
//                 tokens before it (for ADFEA its group token follows with the same E, maybe
//                 in the next span: neither reads the other); a group token writes slots[E].
//                 Nobody loops over a line.
//   4. tp_finish (row-width range), tp_mod.
// What is not certain defers the chunk to the host parser (H_BAD / H_DEFER): a token longer
// than 64 bytes, a '#' opening a line (the host skips such lines), a label, key or (slots
// kept) group the scanners of textnum.h reject, a group outside [0, 2^31), a line of 1 or 2
// tokens, an ADFEA line that ends on a key, an ADFEA ':' before the first token of a line
// (the host does not take such a line for blank). Lines without a token are skipped as the
// host skips blank lines. Without slots the ADFEA group tokens are not scanned (the host does
// not look at them either).
//
// Safety on arbitrary bytes as in textparse.hip: reads clamped to n, sizes from the count
// pass and checked before anything is emitted (sticky H_CAP), every emitted index guarded,
// every token loop bounded by textnum::kMaxTok + 1.
#include "textparse.cuh"

namespace psamd {

namespace {

// per-span summary (ad_count -> ad_scan) and per-span bases (ad_scan -> ad_emit)
enum { S_FN, S_HEAD, S_NLAB, S_NENT, S_WORDS = 4 };
enum { B_LAB, B_ENT, B_CARRY, B_WORDS = 4 };

// Tokens since the last '\n' as a function of the carry-in: bit 31 set, the text holds a
// newline and the low bits are the tokens behind its last one; clear, the low bits are
// added to the carry-in. (A chunk is <= 2^30 bytes: counts stay below 2^30.)
struct TokFn {
  static constexpr uint32_t ident = 0;
  static constexpr uint32_t kNl = 1u << 31;
  __device__ static uint32_t op(uint32_t l, uint32_t r) { return (r & kNl) ? r : l + r; }
};
__device__ __forceinline__ uint32_t tokfn_apply(uint32_t fn, uint32_t in) {
  return (fn & TokFn::kNl) ? (fn & ~TokFn::kNl) : in + fn;
}

// The grammar as functions of a token's index in its line. kAd: ADFEA, else TERAFEA.
template <bool kAd>
struct Gram {
  __device__ static bool sep(uint32_t c) {
    return c == ' ' || c == '\t' || c == '\r' || (kAd && c == ':');
  }
  static constexpr uint32_t kLab = kAd ? 2u : 0u;
  __device__ static bool is_lab(uint32_t t) { return t == kLab; }
  __device__ static bool is_key(uint32_t t) { return t >= 3u && (!kAd || (t & 1u)); }
  __device__ static bool is_ent(uint32_t t) { return kAd ? (t >= 4u && !(t & 1u)) : t >= 3u; }
  // labels / entry tokens among the line indices [0, x)
  __device__ static uint32_t labs_below(uint32_t x) { return x > kLab ? 1u : 0u; }
  __device__ static uint32_t ents_below(uint32_t x) {
    return x < 3u ? 0u : (kAd ? (x - 3u) >> 1 : x - 3u);
  }
  // a complete line of T tokens the host does not turn into a plain example
  __device__ static bool line_bad(uint32_t T) {
    return T == 1u || T == 2u || (kAd && T >= 4u && !(T & 1u));
  }
};

struct AdThread {
  uint32_t ts;                  // token starts among this thread's 16 bytes
  uint32_t first, lab, key, ent;  // of them: line index 0, labels, keys, entry tokens
  uint32_t anom;                // a bad line end or an early ':' among the 16 bytes
  uint32_t lab_excl, ent_excl;  // labels / entry tokens of the span before this thread
};
struct AdBlock {
  uint32_t fn, head, nlab, nent;
};

// Loads and classifies one span. kCount: the carry is not known, the tokens before the
// span's first '\n' are counted (blk.head) and not classified; else `carry` is the line
// index of the span's first token start.
template <bool kAd, bool kCount>
__device__ __forceinline__ void ad_classify(const uint8_t* __restrict__ text, int64_t n,
                                            int64_t base, uint8_t* lds_text, uint32_t* lds_scan,
                                            uint32_t carry, AdThread& t, AdBlock& blk) {
  using G = Gram<kAd>;
  uint32_t w[4];
  const uint32_t prev = tp_load_span(text, n, base, lds_text, w);
  uint32_t nl = 0, tk = 0, col = 0;
#pragma unroll
  for (int k = 0; k < kTpBytes; ++k) {
    const uint32_t c = (w[k >> 2] >> (8 * (k & 3))) & 0xffu;
    const uint32_t is_nl = c == '\n';
    nl |= is_nl << k;
    col |= (uint32_t)(c == ':') << k;
    tk |= (uint32_t)!(is_nl | (uint32_t)G::sep(c)) << k;
  }
  const uint32_t p_tok = !(prev == '\n' || G::sep(prev));
  const uint32_t ts = tk & ~((tk << 1) | p_tok) & 0xffffu;

  uint32_t fn;
  if (nl) {
    const int top = 31 - __clz((int)nl);
    fn = TokFn::kNl | (uint32_t)__popc(ts >> (top + 1));
  } else {
    fn = (uint32_t)__popc(ts);
  }
  uint32_t fn_tot;
  const uint32_t fn_ex = tp_block_scan<TokFn>(fn, lds_scan, &fn_tot);

  bool head = kCount && !(fn_ex & TokFn::kNl);
  uint32_t idx = tokfn_apply(fn_ex, carry);
  uint32_t first = 0, lab = 0, key = 0, ent = 0, anom = 0, h = 0;
#pragma unroll
  for (int k = 0; k < kTpBytes; ++k) {
    const uint32_t bit = 1u << k;
    if (ts & bit) {
      if (head) {
        ++h;
      } else {
        if (idx == 0u) first |= bit;
        if (G::is_lab(idx)) lab |= bit;
        if (G::is_key(idx)) key |= bit;
        if (G::is_ent(idx)) ent |= bit;
      }
      ++idx;
    }
    if (kAd && !kCount && (col & bit) && idx == 0u) anom = 1u;
    if (nl & bit) {
      if (!kCount && G::line_bad(idx)) anom = 1u;
      idx = 0u;
      head = false;
    }
  }

  // labels << 16 | entry tokens: each count is <= 8192 per span
  uint32_t c_tot, h_tot = 0;
  const uint32_t c_ex =
      tp_block_scan<Sum>(((uint32_t)__popc(lab) << 16) | (uint32_t)__popc(ent), lds_scan, &c_tot);
  if (kCount) (void)tp_block_scan<Sum>(h, lds_scan, &h_tot);

  t.ts = ts;
  t.first = first;
  t.lab = lab;
  t.key = key;
  t.ent = ent;
  t.anom = anom;
  t.lab_excl = c_ex >> 16;
  t.ent_excl = c_ex & 0xffffu;
  blk.fn = fn_tot;
  blk.head = h_tot;
  blk.nlab = c_tot >> 16;
  blk.nent = c_tot & 0xffffu;
}

template <bool kAd>
__global__ void __launch_bounds__(kTpBlk) ad_count_kernel(const uint8_t* __restrict__ text,
                                                          int64_t n, int32_t* __restrict__ sum) {
  __shared__ __attribute__((aligned(16))) uint8_t lds_text[kTpSpan];
  __shared__ uint32_t lds_scan[kTpWaves + 1];
  AdThread t;
  AdBlock b;
  ad_classify<kAd, true>(text, n, (int64_t)blockIdx.x * kTpSpan, lds_text, lds_scan, 0u, t, b);
  if (threadIdx.x == 0) {
    int32_t* s = sum + (int64_t)blockIdx.x * S_WORDS;
    s[S_FN] = (int32_t)b.fn;
    s[S_HEAD] = (int32_t)b.head;
    s[S_NLAB] = (int32_t)b.nlab;
    s[S_NENT] = (int32_t)b.nent;
  }
}

// One workgroup: span carries and bases by workgroup scans over 1024 span summaries at a
// time (the running totals are the same in every thread), then the header.
template <bool kAd>
__global__ void __launch_bounds__(kTpBlk) ad_scan_kernel(const int32_t* __restrict__ sum,
                                                         int32_t* __restrict__ bases, int64_t nb,
                                                         int64_t row0, int64_t nnz0,
                                                         int64_t cap_rows, int64_t cap_rp,
                                                         int64_t cap_nnz,
                                                         int64_t* __restrict__ row_ptr,
                                                         int32_t* __restrict__ hdr) {
  using G = Gram<kAd>;
  __shared__ uint32_t lds_scan[kTpWaves + 1];
  uint32_t lab = 0, ent = 0, state = 0;
  for (int64_t c = 0; c < nb; c += kTpBlk) {
    const int64_t i = c + threadIdx.x;
    const bool on = i < nb;
    const int32_t* s = sum + (on ? i : 0) * S_WORDS;
    const uint32_t fn = on ? (uint32_t)s[S_FN] : TokFn::ident;
    const uint32_t h = on ? (uint32_t)s[S_HEAD] : 0u;
    const uint32_t nlab = on ? (uint32_t)s[S_NLAB] : 0u, nent = on ? (uint32_t)s[S_NENT] : 0u;
    uint32_t fn_tot, lab_tot, ent_tot;
    const uint32_t fn_ex = tp_block_scan<TokFn>(fn, lds_scan, &fn_tot);
    const uint32_t in = tokfn_apply(fn_ex, state);  // line index of the span's first token
    const uint32_t hl = G::labs_below(in + h) - G::labs_below(in);
    const uint32_t he = G::ents_below(in + h) - G::ents_below(in);
    const uint32_t lab_ex = tp_block_scan<Sum>(nlab + hl, lds_scan, &lab_tot);
    const uint32_t ent_ex = tp_block_scan<Sum>(nent + he, lds_scan, &ent_tot);
    if (on) {
      int32_t* o = bases + i * B_WORDS;
      o[B_LAB] = (int32_t)(lab + lab_ex);
      o[B_ENT] = (int32_t)(ent + ent_ex);
      o[B_CARRY] = (int32_t)in;
    }
    lab += lab_tot;
    ent += ent_tot;
    state = tokfn_apply(fn_tot, state);
  }
  // (a last line that ends with the text and not with a '\n': its end is checked here when
  // the text fills its last span, by the padding newline in ad_emit otherwise)
  if (threadIdx.x == 0)
    tp_write_header(lab, ent, G::line_bad(state) ? 1u : 0u, row0, nnz0, cap_rows, cap_rp,
                    cap_nnz, row_ptr, hdr);
}

// kSlots: write every entry's group (ADFEA: its group token, TERAFEA: key >> 54).
template <bool kAd, bool kSlots>
__global__ void __launch_bounds__(kTpBlk) ad_emit_kernel(
    const uint8_t* __restrict__ text, int64_t n, const int32_t* __restrict__ bases, int64_t row0,
    int64_t nnz0, int64_t cap_rows, int64_t cap_nnz, float* __restrict__ labels,
    int64_t* __restrict__ row_ptr, uint64_t* __restrict__ keys, int32_t* __restrict__ slots,
    int32_t* __restrict__ hdr) {
  using G = Gram<kAd>;
  __shared__ __attribute__((aligned(16))) uint8_t lds_text[kTpSpan];
  __shared__ uint32_t lds_scan[kTpWaves + 1];
  if (hdr[H_CAP]) return;  // (uniform: set before this launch)
  const int32_t* bs = bases + (int64_t)blockIdx.x * B_WORDS;
  const int64_t base = (int64_t)blockIdx.x * kTpSpan;
  AdThread t;
  AdBlock b;
  ad_classify<kAd, false>(text, n, base, lds_text, lds_scan, (uint32_t)bs[B_CARRY], t, b);
  const int64_t rows = hdr[H_ROWS], nnz = hdr[H_NNZ];
  int64_t R = (int64_t)bs[B_LAB] + t.lab_excl;  // labels before the next token: its row
  int64_t E = (int64_t)bs[B_ENT] + t.ent_excl;  // entry tokens before it: its entry
  int bad = 0, defer = (int)t.anom;
  uint32_t r = t.ts;
  while (r) {
    const int i = __ffs((int)r) - 1;
    r &= r - 1;
    const int off = threadIdx.x * kTpBytes + i;
    const bool is_lab = (t.lab >> i) & 1u, is_key = (t.key >> i) & 1u, is_ent = (t.ent >> i) & 1u;
    int lim;
    const uint8_t* p = tp_token_window(text, n, base, off, lds_text, &lim);
    int len = 0;
    for (; len < lim; ++len) {
      const uint32_t c = p[len];
      if (c == '\n' || G::sep(c)) break;
    }
    int st = textnum::kOk;
    if (len > textnum::kMaxTok || (((t.first >> i) & 1u) && p[0] == '#')) {
      st = textnum::kDefer;
    } else if (is_lab) {
      int64_t c = 0;
      st = textnum::scan_i64(p, len, &c);
      if (st == textnum::kOk && R < rows && in_range(row0 + R, cap_rows)) {
        labels[row0 + R] = c > 0 ? 1.f : -1.f;
        row_ptr[row0 + R] = nnz0 + E;
      }
    } else if (is_key) {
      uint64_t key = 0;
      st = textnum::scan_u64(p, len, &key);
      if (st == textnum::kOk && E < nnz && in_range(nnz0 + E, cap_nnz)) {
        keys[nnz0 + E] = key;  // (raw: tp_mod reduces)
        if (!kAd && kSlots) slots[nnz0 + E] = (int32_t)(key >> 54);
      }
    } else if (kAd && kSlots && is_ent) {
      int64_t v = 0;
      st = textnum::scan_i64(p, len, &v);
      if (st == textnum::kOk && (v < 0 || v >= ((int64_t)1 << 31))) st = textnum::kDefer;
      if (st == textnum::kOk && E < nnz && in_range(nnz0 + E, cap_nnz)) slots[nnz0 + E] = (int32_t)v;
    }
    R += is_lab;
    E += is_ent;
    bad += st == textnum::kBad;
    defer += st == textnum::kDefer;
  }
  tp_report<false>(bad, defer, 0, hdr);
}

template <bool kAd>
void ad_launch_as(const uint8_t* text, int64_t n, uint64_t hash_mod, const TextOut& o,
                  int32_t* work, hipStream_t st) {
  const int64_t nb = (n + kTpSpan - 1) / kTpSpan;
  int32_t* sum = work;
  int32_t* bases = work + nb * S_WORDS;
  ad_count_kernel<kAd><<<(unsigned)nb, kTpBlk, 0, st>>>(text, n, sum);
  ad_scan_kernel<kAd><<<1, kTpBlk, 0, st>>>(sum, bases, nb, o.row0, o.nnz0, o.cap_rows, o.cap_rp,
                                            o.cap_nnz, o.row_ptr, o.hdr);
  const auto emit = o.slots ? ad_emit_kernel<kAd, true> : ad_emit_kernel<kAd, false>;
  emit<<<(unsigned)nb, kTpBlk, 0, st>>>(text, n, bases, o.row0, o.nnz0, o.cap_rows, o.cap_nnz,
                                        o.labels, o.row_ptr, o.keys, o.slots, o.hdr);
  tp_finish(o, n, false, hash_mod, st);
}

}  // namespace

int64_t ad_work_words(int64_t n) { return ((n + kTpSpan - 1) / kTpSpan) * (S_WORDS + B_WORDS); }

// Behind textparse()'s checks (textparse.hip). adfea: ADFEA, else TERAFEA.
void ad_launch(const uint8_t* text, int64_t n, bool adfea, uint64_t hash_mod, const TextOut& o,
               int32_t* work, hipStream_t st) {
  if (adfea) ad_launch_as<true>(text, n, hash_mod, o, work, st);
  else ad_launch_as<false>(text, n, hash_mod, o, work, st);
}

}  // namespace psamd
