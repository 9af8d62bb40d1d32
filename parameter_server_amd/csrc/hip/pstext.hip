// SPARSE_BINARY / SPARSE text ("label; grp key key ...; grp key:val ...;") -> CSR minibatch
// arrays and per-feature slot ids on the device (gfx950), the device half of
// csrc/core/data.cc parse_ps with parse_range. A strict fast path next to textparse.hip,
// with the same decomposition (textparse.cuh): 16 KiB of text per 1024-thread workgroup,
// count -> scan -> emit -> finish in separate launches, no hand-off between workgroups.
//
// Token bytes are everything except '\n', ';', blank, tab and CR; a token belongs to the
// thread that holds its first byte. A token is the LABEL when no token precedes it on its
// line, a group HEAD when it is the first token since a ';' on a line that has its label,
// else a FEATURE. Three carries decide that, each a function a | (b & carry_in) of the
// state of the text before (they compose associatively, one packed word: Fn3):
//   L  the line holds a token                      (set by a token, reset by '\n')
//   G  the current group holds a token             (set by a token, reset by ';' and '\n')
//   S  the line has seen a ';'                     (set by ';', reset by '\n')
// Feature index of a feature token = tokens before it - labels - heads up to it, so
// row_ptr falls out of the scans before any number is parsed.
//   1. ps_count   classifies its span as if the text before it ended inside a group with
//                 features (carry L = G = S = 1) and reports token / label / head counts,
//                 the span's Fn3, and whether its first token starts before any '\n' or
//                 ';' of the span (amb): only that token's class depends on the carry.
//   2. ps_scan    one workgroup: span bases and true carries, the amb token booked as a
//                 label (carry !L) or a head (L, S, !G), header, capacity check.
//   3. ps_emit    re-classifies with the true carries; one thread per token parses it and
//                 writes label and row offset, or key / value at the feature's position.
//                 With slots: a feature writes its group's ordinal, the head token writes
//                 group_slot[ordinal] (a group may be longer than a span: nobody loops
//                 over a group).
//   4. ps_gather  slots[j] = group_slot[slots[j]] (with slots only), tp_finish (row-width
//                 range), tp_mod.
// What is not certain defers the chunk to the host parser (H_BAD / H_DEFER): a token longer
// than 64 bytes, a number outside textnum's exact domain, a '#' label, a second token
// before the line's first ';' (the host ignores it), a ';' on a line without a token (a bad
// line on the host), a ':' in a SPARSE_BINARY feature (the host splits there), a SPARSE
// feature that is not exactly digits:number (the host pairs tokens across blanks), a head
// that is no integer in [0, 2^31) when slots are wanted. Without slots the head's bytes are
// not scanned (the host does not look at them either).
//
// Safety on arbitrary bytes as in textparse.hip: reads clamped to n, sizes from the count
// pass and checked before anything is emitted (sticky H_CAP), every emitted index guarded,
// every token loop bounded by textnum::kMaxTok + 1.
#include "textparse.cuh"

namespace psamd {

namespace {

// per-span summary (ps_count -> ps_scan) and per-span bases (ps_scan -> ps_emit)
enum { S_NTOK, S_NLAB, S_NHEAD, S_AMB, S_FN, S_WORDS = 8 };
enum { B_TOK, B_LAB, B_HEAD, B_STATE, B_WORDS = 4 };
enum { A_NGROUPS, A_WORDS = 16 };  // words between the bases and group_slot

// The carries L (bit 0), G (bit 1), S (bit 2) as functions of the carry-in, a | b << 3.
struct Fn3 {
  static constexpr uint32_t ident = 7u << 3;
  __device__ static uint32_t op(uint32_t l, uint32_t r) {
    const uint32_t a = (r & 7u) | ((r >> 3) & l & 7u), b = (r >> 3) & (l >> 3) & 7u;
    return a | (b << 3);
  }
};
__device__ __forceinline__ uint32_t fn3_apply(uint32_t fn, uint32_t in) {
  return (fn & 7u) | ((fn >> 3) & in & 7u);
}
// One carry over 16 bytes: set / reset byte masks -> a | b << 1.
__device__ __forceinline__ uint32_t fn_of(uint32_t set, uint32_t reset) {
  if (reset) {
    const int top = 31 - __clz((int)reset);
    return (set >> (top + 1)) ? 1u : 0u;  // b = 0
  }
  return (set ? 1u : 0u) | 2u;  // b = 1
}

struct PsThread {
  uint32_t ts;         // token starts among this thread's 16 bytes
  uint32_t lab, head;  // of them: labels, group heads
  uint32_t early;      // of them: a second token before the line's first ';'
  uint32_t semibad;    // a ';' on a line that holds no token
  uint32_t tok_excl, lab_excl, head_excl;  // counts of the span before this thread
};
struct PsBlock {
  uint32_t ntok, nlab, nhead, amb, fn;
};

// Loads and classifies one span under the carry (L | G << 1 | S << 2) of the text before it.
__device__ __forceinline__ void ps_classify(const uint8_t* __restrict__ text, int64_t n,
                                            int64_t base, uint8_t* lds_text, uint32_t* lds_scan,
                                            uint32_t carry, PsThread& t, PsBlock& blk) {
  uint32_t w[4];
  const uint32_t prev = tp_load_span(text, n, base, lds_text, w);
  uint32_t nl = 0, semi = 0, tk = 0;
#pragma unroll
  for (int k = 0; k < kTpBytes; ++k) {
    const uint32_t c = (w[k >> 2] >> (8 * (k & 3))) & 0xffu;
    const uint32_t is_nl = c == '\n', is_semi = c == ';';
    const uint32_t is_bl = (c == ' ') | (c == '\t') | (c == '\r');
    nl |= is_nl << k;
    semi |= is_semi << k;
    tk |= (uint32_t)!(is_nl | is_semi | is_bl) << k;
  }
  const uint32_t p_tok =
      !(prev == '\n' || prev == ';' || prev == ' ' || prev == '\t' || prev == '\r');
  const uint32_t ts = tk & ~((tk << 1) | p_tok) & 0xffffu;

  const uint32_t fl = fn_of(tk, nl), fg = fn_of(tk, nl | semi), fs = fn_of(semi, nl);
  const uint32_t fn = (fl & 1u) | ((fg & 1u) << 1) | ((fs & 1u) << 2) | ((fl >> 1) << 3) |
                      ((fg >> 1) << 4) | ((fs >> 1) << 5);
  uint32_t fn_tot;
  const uint32_t fn_ex = tp_block_scan<Fn3>(fn, lds_scan, &fn_tot);
  const uint32_t in = fn3_apply(fn_ex, carry);

  uint32_t L = in & 1u, G = (in >> 1) & 1u, S = (in >> 2) & 1u;
  uint32_t lab = 0, head = 0, early = 0, semibad = 0;
#pragma unroll
  for (int k = 0; k < kTpBytes; ++k) {
    const uint32_t bit = 1u << k;
    if (ts & bit) {
      if (!L) lab |= bit;
      else if (!S) early |= bit;
      else if (!G) head |= bit;
    }
    if (tk & bit) L = G = 1u;
    if (semi & bit) {
      semibad |= L ^ 1u;
      G = 0u;
      S = 1u;
    }
    if (nl & bit) L = G = S = 0u;
  }
  // the span's first token start, when neither a '\n', a ';' nor the tail of a token of
  // the text before precedes it in the span: the one token whose class the carry decides
  uint32_t amb = 0;
  if (ts) {
    const int i0 = __ffs((int)ts) - 1;
    if (!((nl | semi | tk) & ((1u << i0) - 1u)) && (fn_ex & (1u << 4)) && !(fn_ex & 2u)) amb = 1u;
  }

  // token starts << 16 | amb << 15 | labels, then heads: each count is <= 8192 per span
  uint32_t c1_tot, c2_tot;
  const uint32_t c1_ex = tp_block_scan<Sum>(
      ((uint32_t)__popc(ts) << 16) | (amb << 15) | (uint32_t)__popc(lab), lds_scan, &c1_tot);
  const uint32_t c2_ex = tp_block_scan<Sum>((uint32_t)__popc(head), lds_scan, &c2_tot);

  t.ts = ts;
  t.lab = lab;
  t.head = head;
  t.early = early;
  t.semibad = semibad;
  t.tok_excl = c1_ex >> 16;
  t.lab_excl = c1_ex & 0x7fffu;
  t.head_excl = c2_ex;
  blk.ntok = c1_tot >> 16;
  blk.amb = (c1_tot >> 15) & 1u;
  blk.nlab = c1_tot & 0x7fffu;
  blk.nhead = c2_tot;
  blk.fn = fn_tot;
}

__global__ void __launch_bounds__(kTpBlk) ps_count_kernel(const uint8_t* __restrict__ text,
                                                          int64_t n, int32_t* __restrict__ sum) {
  __shared__ __attribute__((aligned(16))) uint8_t lds_text[kTpSpan];
  __shared__ uint32_t lds_scan[kTpWaves + 1];
  PsThread t;
  PsBlock b;
  ps_classify(text, n, (int64_t)blockIdx.x * kTpSpan, lds_text, lds_scan, 7u, t, b);
  if (threadIdx.x == 0) {
    int32_t* s = sum + (int64_t)blockIdx.x * S_WORDS;
    s[S_NTOK] = (int32_t)b.ntok;
    s[S_NLAB] = (int32_t)b.nlab;
    s[S_NHEAD] = (int32_t)b.nhead;
    s[S_AMB] = (int32_t)b.amb;
    s[S_FN] = (int32_t)b.fn;
  }
}

// One workgroup: span bases and carries by workgroup scans over 1024 span summaries at a
// time (the running totals are the same in every thread), then the header.
__global__ void __launch_bounds__(kTpBlk) ps_scan_kernel(const int32_t* __restrict__ sum,
                                                         int32_t* __restrict__ bases, int64_t nb,
                                                         int64_t row0, int64_t nnz0,
                                                         int64_t cap_rows, int64_t cap_rp,
                                                         int64_t cap_nnz,
                                                         int64_t* __restrict__ row_ptr,
                                                         int32_t* __restrict__ aux,
                                                         int32_t* __restrict__ hdr) {
  __shared__ uint32_t lds_scan[kTpWaves + 1];
  uint32_t tok = 0, lab = 0, head = 0, state = 0;
  for (int64_t c = 0; c < nb; c += kTpBlk) {
    const int64_t i = c + threadIdx.x;
    const bool on = i < nb;
    const int32_t* s = sum + (on ? i : 0) * S_WORDS;
    const uint32_t ntok = on ? (uint32_t)s[S_NTOK] : 0u, nlab = on ? (uint32_t)s[S_NLAB] : 0u;
    const uint32_t nhead = on ? (uint32_t)s[S_NHEAD] : 0u, amb = on ? (uint32_t)s[S_AMB] : 0u;
    const uint32_t fn = on ? ((uint32_t)s[S_FN] & 63u) : Fn3::ident;
    uint32_t fn_tot, tok_tot, lab_tot, head_tot;
    const uint32_t fn_ex = tp_block_scan<Fn3>(fn, lds_scan, &fn_tot);
    const uint32_t in = fn3_apply(fn_ex, state);
    const uint32_t L = in & 1u, G = (in >> 1) & 1u, S = (in >> 2) & 1u;
    const uint32_t tok_ex = tp_block_scan<Sum>(ntok, lds_scan, &tok_tot);
    const uint32_t lab_ex = tp_block_scan<Sum>(nlab + ((amb && !L) ? 1u : 0u), lds_scan, &lab_tot);
    const uint32_t head_ex =
        tp_block_scan<Sum>(nhead + ((amb && L && S && !G) ? 1u : 0u), lds_scan, &head_tot);
    if (on) {
      int32_t* o = bases + i * B_WORDS;
      o[B_TOK] = (int32_t)(tok + tok_ex);
      o[B_LAB] = (int32_t)(lab + lab_ex);
      o[B_HEAD] = (int32_t)(head + head_ex);
      o[B_STATE] = (int32_t)in;
    }
    tok += tok_tot;
    lab += lab_tot;
    head += head_tot;
    state = fn3_apply(fn_tot, state);
  }
  if (threadIdx.x == 0) {
    aux[A_NGROUPS] = (int32_t)head;
    tp_write_header(lab, (int64_t)tok - (int64_t)lab - (int64_t)head, 0u, row0, nnz0, cap_rows,
                    cap_rp, cap_nnz, row_ptr, hdr);
  }
}

// kValued: SPARSE (key:value features), else SPARSE_BINARY. kSlots: read the group heads.
template <bool kValued, bool kSlots>
__global__ void __launch_bounds__(kTpBlk) ps_emit_kernel(
    const uint8_t* __restrict__ text, int64_t n, const int32_t* __restrict__ bases, int64_t row0,
    int64_t nnz0, int64_t cap_rows, int64_t cap_nnz, float* __restrict__ labels,
    int64_t* __restrict__ row_ptr, uint64_t* __restrict__ keys, float* __restrict__ vals,
    int32_t* __restrict__ slots, int32_t* __restrict__ group_slot, int64_t cap_groups,
    int32_t* __restrict__ hdr) {
  __shared__ __attribute__((aligned(16))) uint8_t lds_text[kTpSpan];
  __shared__ uint32_t lds_scan[kTpWaves + 1];
  if (hdr[H_CAP]) return;  // (uniform: set before this launch)
  const int32_t* bs = bases + (int64_t)blockIdx.x * B_WORDS;
  const int64_t base = (int64_t)blockIdx.x * kTpSpan;
  PsThread t;
  PsBlock b;
  ps_classify(text, n, base, lds_text, lds_scan, (uint32_t)bs[B_STATE] & 7u, t, b);
  const int64_t rows = hdr[H_ROWS], nnz = hdr[H_NNZ];
  int64_t T = (int64_t)bs[B_TOK] + t.tok_excl;    // global index of the next token
  int64_t L = (int64_t)bs[B_LAB] + t.lab_excl;    // labels before it
  int64_t Hd = (int64_t)bs[B_HEAD] + t.head_excl;  // group heads before it
  int bad = 0, defer = t.semibad ? 1 : 0, nonunit = 0;
  uint32_t r = t.ts;
  while (r) {
    const int i = __ffs((int)r) - 1;
    r &= r - 1;
    const int off = threadIdx.x * kTpBytes + i;
    const bool is_lab = (t.lab >> i) & 1u, is_head = (t.head >> i) & 1u;
    if (is_lab) ++L;
    if (is_head) ++Hd;
    const int64_t R = L - 1;         // this token's row
    const int64_t pos = T - L - Hd;  // a feature token's index among the features
    ++T;
    int lim;
    const uint8_t* p = tp_token_window(text, n, base, off, lds_text, &lim);
    int len = 0, colon = -1, ncolon = 0;
    for (; len < lim; ++len) {
      const uint32_t c = p[len];
      if (c == '\n' || c == ';' || c == ' ' || c == '\t' || c == '\r') break;
      if (c == ':') {
        if (colon < 0) colon = len;
        ++ncolon;
      }
    }
    int st = textnum::kOk;
    if (len > textnum::kMaxTok || R < 0 || R >= rows || ((t.early >> i) & 1u)) {
      st = textnum::kDefer;
    } else if (is_lab) {
      int64_t c = 0;
      st = p[0] == '#' ? (int)textnum::kDefer : textnum::scan_i64(p, len, &c);
      if (st == textnum::kOk && in_range(row0 + R, cap_rows)) {
        labels[row0 + R] = c > 0 ? 1.f : -1.f;
        row_ptr[row0 + R] = nnz0 + pos + 1;  // (pos counts this label: the features before it)
      }
    } else if (is_head) {
      if (kSlots) {
        int64_t v = 0;
        st = textnum::scan_i64(p, len, &v);
        if (st == textnum::kOk && (v < 0 || v >= ((int64_t)1 << 31))) st = textnum::kDefer;
        if (st == textnum::kOk && in_range(Hd - 1, cap_groups)) group_slot[Hd - 1] = (int32_t)v;
      }
    } else {
      uint64_t key = 0;
      float v = 1.f;
      if (kValued) {
        if (ncolon != 1 || colon == 0 || colon == len - 1) {
          st = textnum::kDefer;
        } else {
          st = textnum::scan_u64(p, colon, &key);
          if (st == textnum::kOk) st = textnum::scan_f32(p + colon + 1, len - colon - 1, &v);
        }
      } else {
        st = ncolon ? (int)textnum::kDefer : textnum::scan_u64(p, len, &key);
      }
      if (st == textnum::kOk && pos >= 0 && pos < nnz && in_range(nnz0 + pos, cap_nnz)) {
        keys[nnz0 + pos] = key;  // (raw: tp_mod reduces)
        if (kValued) {
          vals[nnz0 + pos] = v;
          if (v != 1.f) nonunit = 1;
        }
        if (kSlots) slots[nnz0 + pos] = (int32_t)(Hd - 1);  // (the group's ordinal: ps_gather)
      }
    }
    bad += st == textnum::kBad;
    defer += st == textnum::kDefer;
  }
  tp_report(bad, defer, nonunit, hdr);
}

// slots[j]: the ordinal of feature j's group -> the value of that group's head.
__global__ void __launch_bounds__(256) ps_gather_kernel(int32_t* __restrict__ slots, int64_t nnz0,
                                                        const int32_t* __restrict__ group_slot,
                                                        int64_t cap_groups,
                                                        const int32_t* __restrict__ aux,
                                                        const int32_t* __restrict__ hdr) {
  if (hdr[H_CAP]) return;
  const int64_t nnz = hdr[H_NNZ];
  int64_t ng = aux[A_NGROUPS];
  ng = ng < cap_groups ? ng : cap_groups;
  for (int64_t j = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; j < nnz;
       j += (int64_t)gridDim.x * blockDim.x) {
    const int64_t o = slots[nnz0 + j];
    slots[nnz0 + j] = (o >= 0 && o < ng) ? group_slot[o] : 0;
  }
}

inline int64_t ps_cap_groups(int64_t n) { return n / 2 + 2; }  // (a head every two bytes)

}  // namespace

int64_t ps_work_words(int64_t n) {
  return ((n + kTpSpan - 1) / kTpSpan) * (S_WORDS + B_WORDS) + A_WORDS + ps_cap_groups(n);
}

// Behind textparse()'s checks (textparse.hip). valued: SPARSE, else SPARSE_BINARY.
void ps_launch(const uint8_t* text, int64_t n, bool valued, uint64_t hash_mod, const TextOut& o,
               int32_t* work, hipStream_t st) {
  const int64_t nb = (n + kTpSpan - 1) / kTpSpan;
  int32_t* sum = work;
  int32_t* bases = work + nb * S_WORDS;
  int32_t* aux = bases + nb * B_WORDS;
  int32_t* group_slot = aux + A_WORDS;
  const int64_t cap_groups = ps_cap_groups(n);
  ps_count_kernel<<<(unsigned)nb, kTpBlk, 0, st>>>(text, n, sum);
  ps_scan_kernel<<<1, kTpBlk, 0, st>>>(sum, bases, nb, o.row0, o.nnz0, o.cap_rows, o.cap_rp,
                                    o.cap_nnz, o.row_ptr, aux, o.hdr);
  const auto emit = valued ? (o.slots ? ps_emit_kernel<true, true> : ps_emit_kernel<true, false>)
                           : (o.slots ? ps_emit_kernel<false, true> : ps_emit_kernel<false, false>);
  emit<<<(unsigned)nb, kTpBlk, 0, st>>>(text, n, bases, o.row0, o.nnz0, o.cap_rows, o.cap_nnz,
                                        o.labels, o.row_ptr, o.keys, o.vals, o.slots, group_slot,
                                        cap_groups, o.hdr);
  if (o.slots)
    ps_gather_kernel<<<tp_fgrid(n), 256, 0, st>>>(o.slots, o.nnz0, group_slot, cap_groups, aux,
                                                  o.hdr);
  tp_finish(o, n, false, hash_mod, st);
}

}  // namespace psamd
