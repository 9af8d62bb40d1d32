// LIBSVM / CRITEO text -> CSR minibatch arrays on the device (gfx950), the device half of
// csrc/core/data.cc parse_libsvm / parse_criteo. A strict fast path: whatever the kernels
// do not want to decide (a malformed line, a '#' comment, a number outside the exact
// domain of ../core/textnum.h, a token longer than 64 bytes) raises the header's bad /
// deferred counts and the caller re-parses the whole chunk on the host.
//
// Token-parallel, so the work does not depend on line length. Every workgroup owns one
// 16 KiB span of text (1024 threads x one 16-byte load each, staged in LDS); a token
// belongs to the thread that holds its first byte. Four launches, no hand-off between
// workgroups inside a launch:
//   1. tp_count   byte classes -> per-span summary: token starts, row starts ("label"
//                 tokens: the first token of a line), and the two carries a span needs
//                 from the text before it: "does the current line already hold a token"
//                 (as a function a | (b & carry_in), which composes associatively) and,
//                 for CRITEO, "tabs since the last newline" (the field number of a token
//                 is a count of tabs, not of tokens: empty fields shift it).
//   2. tp_scan    one workgroup scans the span summaries: token / row bases and carries
//                 per span, the header (rows, nnz, capacity check) and the last row_ptr.
//   3. tp_emit    re-classifies its span with the carries, then one thread per token
//                 parses it (from LDS; from global memory when it runs past the span)
//                 and writes the label and row offset, or the key and value, at the
//                 token's final position: token T of row R is feature T - R - 1 overall,
//                 so row_ptr falls out of the two scans before any number is parsed.
//   4. tp_finish  non-decreasing LIBSVM indices (a descent is legal only at a row start:
//                 only descents search row_ptr), min / max row width, then keys mod
//                 hash_mod in a launch of its own (tp_mod: the check reads raw keys).
// The same count / scan / emit launches read key<TAB>weight model files (modeltext_parse,
// an internal format: rows are a key token and a weight token, no row offsets, no finish).
// Text traffic: the text is read twice (count, emit); outputs are written once, the keys
// re-read once (and rewritten when hash_mod != 0), row_ptr re-read once.
//
// Safety on arbitrary bytes: every text read is clamped to n (bytes past it read as
// '\n'), every output size comes from the counting pass and is checked against the
// capacities before anything is emitted (sticky H_CAP), every emitted index is guarded,
// and every loop over a token is bounded by textnum::kMaxTok + 1.
#include "textparse.cuh"

#include <stdexcept>
#include <string>

namespace psamd {

namespace {

// Internal: key<TAB>weight model lines (modeltext_parse below; not a data.TEXT_FORMATS id).
// Tokens as in LIBSVM; a row is a key token and its weight token, nothing else.
constexpr int kFmtModel = 100;

// per-span summary (tp_count -> tp_scan) and per-span bases (tp_scan -> tp_emit)
enum { S_NTOK, S_LAB1, S_AMB, S_FN, S_TAB, S_ANOM, S_WORDS = 8 };
enum { B_TOK, B_LAB, B_HAS, B_TABS, B_WORDS = 4 };

// tabs since the last newline: count | saw_newline << 31.
struct TabSeg {
  static constexpr uint32_t ident = 0;
  __device__ static uint32_t op(uint32_t l, uint32_t r) {
    return (r >> 31) ? r : ((l & 0x80000000u) | ((l & 0x7fffffffu) + r));
  }
};

struct TpThread {
  uint32_t ts;        // token starts among this thread's 16 bytes
  uint32_t lab;       // of them: first token of a line (a row's label)
  uint32_t nl, tab;   // newline / tab bytes
  uint32_t tok_excl;  // token starts of the span before this thread
  uint32_t lab_excl;  // row starts of the span before this thread
  uint32_t tabs_in;   // CRITEO: tabs since the last newline at this thread's first byte
};
struct TpBlock {
  uint32_t ntok, nlab, amb, fn, tabseg, anom;
};

// Loads and classifies one span. carry_has / carry_tabs: the state of the text before the
// span (tp_count passes 1 / 0 and reports through blk.amb whether the span's first token
// start would be a row start under carry 0).
template <int kFmt>
__device__ __forceinline__ void tp_classify(const uint8_t* __restrict__ text, int64_t n,
                                            int64_t base, uint8_t* lds_text, uint32_t* lds_scan,
                                            uint32_t carry_has, uint32_t carry_tabs, TpThread& t,
                                            TpBlock& blk) {
  uint32_t w[4];
  const uint32_t prev = tp_load_span(text, n, base, lds_text, w);

  uint32_t nl = 0, tab = 0, blank = 0, tk = 0;
#pragma unroll
  for (int k = 0; k < kTpBytes; ++k) {
    const uint32_t c = (w[k >> 2] >> (8 * (k & 3))) & 0xffu;
    const uint32_t is_nl = c == '\n', is_tab = c == '\t', is_bl = (c == ' ') | (c == '\r');
    nl |= is_nl << k;
    tab |= is_tab << k;
    blank |= is_bl << k;
    tk |= (uint32_t)!(is_nl | is_tab | is_bl) << k;
  }
  const uint32_t p_nl = prev == '\n', p_tab = prev == '\t', p_bl = (prev == ' ') | (prev == '\r');
  uint32_t ts, anom = 0;
  if (kFmt == kFmtLibsvm || kFmt == kFmtModel) {
    // separators: blank, tab, CR; a token starts after a separator or a newline
    const uint32_t p_tok = !(p_nl | p_tab | p_bl);
    ts = tk & ~((tk << 1) | p_tok);
    if (kFmt == kFmtModel) anom = blank;  // (a blank or CR anywhere: the host decides)
  } else {
    // fields end at tab / newline only; blanks are trimmed at a field's END, so content
    // after a blank inside a field is a malformed field (or a field past the 39th)
    const uint32_t bd = nl | tab;
    ts = tk & ((bd << 1) | (p_nl | p_tab));
    anom = tk & ((blank << 1) | p_bl);
  }
  ts &= 0xffffu;
  anom &= 0xffffu;

  // row starts under carry 0: a token start with no other token start since the last
  // newline; under carry 1 the one before the thread's first newline (amb_bit) is not
  uint32_t lab0 = 0, amb_bit = 0;
  {
    uint32_t r = ts, done = 0;
    bool has = false;
    while (r) {
      const int i = __ffs((int)r) - 1;
      const uint32_t below = (1u << i) - 1u;
      if (nl & below & ~done) has = false;
      if (!has) lab0 |= 1u << i;
      has = true;
      done = below;
      r &= r - 1;
    }
    if (ts) {
      const int i0 = __ffs((int)ts) - 1;
      if (!(nl & ((1u << i0) - 1u))) amb_bit = 1u << i0;
    }
  }
  uint32_t fn;
  if (nl) {
    const int top = 31 - __clz((int)nl);
    fn = (ts >> (top + 1)) ? 1u : 0u;  // b = 0
  } else {
    fn = (ts ? 1u : 0u) | 2u;  // b = 1
  }
  uint32_t fn_tot;
  const uint32_t fn_ex = tp_block_scan<LineFn>(fn, lds_scan, &fn_tot);
  const uint32_t has_in = (fn_ex & 1) | ((fn_ex >> 1) & carry_has & 1);
  const uint32_t lab = has_in ? (lab0 & ~amb_bit) : lab0;
  // (the span's first token start, when no newline of the span precedes it)
  const uint32_t amb_blk = (amb_bit && !(fn_ex & 1) && (fn_ex >> 1)) ? 1u : 0u;

  // token starts << 16 | amb << 15 | row starts: each count is <= 8192 per span
  uint32_t cnt_tot;
  const uint32_t cnt_ex = tp_block_scan<Sum>(
      ((uint32_t)__popc(ts) << 16) | (amb_blk << 15) | (uint32_t)__popc(lab), lds_scan, &cnt_tot);

  t.ts = ts;
  t.lab = lab;
  t.nl = nl;
  t.tab = tab;
  t.tok_excl = cnt_ex >> 16;
  t.lab_excl = cnt_ex & 0x7fffu;
  t.tabs_in = 0;
  blk.ntok = cnt_tot >> 16;
  blk.amb = (cnt_tot >> 15) & 1u;
  blk.nlab = cnt_tot & 0x7fffu;
  blk.fn = fn_tot;
  blk.tabseg = 0;
  blk.anom = 0;
  if (kFmt == kFmtCriteo) {
    uint32_t seg;
    if (nl) {
      const int top = 31 - __clz((int)nl);
      seg = 0x80000000u | (uint32_t)__popc(tab >> (top + 1));
    } else {
      seg = (uint32_t)__popc(tab);
    }
    uint32_t seg_tot;
    const uint32_t seg_ex = tp_block_scan<TabSeg>(seg, lds_scan, &seg_tot);
    t.tabs_in = (seg_ex >> 31) ? (seg_ex & 0x7fffffffu) : carry_tabs + seg_ex;
    blk.tabseg = seg_tot;
    blk.anom = (uint32_t)__syncthreads_or((int)anom) ? 1u : 0u;
  }
  if (kFmt == kFmtModel) blk.anom = (uint32_t)__syncthreads_or((int)anom) ? 1u : 0u;
}

template <int kFmt>
__global__ void __launch_bounds__(kTpBlk) tp_count_kernel(const uint8_t* __restrict__ text,
                                                          int64_t n, int32_t* __restrict__ sum) {
  __shared__ __attribute__((aligned(16))) uint8_t lds_text[kTpSpan];
  __shared__ uint32_t lds_scan[kTpWaves + 1];
  TpThread t;
  TpBlock b;
  tp_classify<kFmt>(text, n, (int64_t)blockIdx.x * kTpSpan, lds_text, lds_scan, 1u, 0u, t, b);
  if (threadIdx.x == 0) {
    int32_t* s = sum + (int64_t)blockIdx.x * S_WORDS;
    s[S_NTOK] = (int32_t)b.ntok;
    s[S_LAB1] = (int32_t)b.nlab;
    s[S_AMB] = (int32_t)b.amb;
    s[S_FN] = (int32_t)b.fn;
    s[S_TAB] = (int32_t)b.tabseg;
    s[S_ANOM] = (int32_t)b.anom;
  }
}

// One workgroup: span bases and carries by workgroup scans over 1024 span summaries at a
// time (the running carries are the same in every thread), then the header, the capacity
// check and the closing row offset.
__global__ void __launch_bounds__(kTpBlk) tp_scan_kernel(const int32_t* __restrict__ sum,
                                                         int32_t* __restrict__ bases, int64_t nb,
                                                         int64_t row0, int64_t nnz0,
                                                         int64_t cap_rows, int64_t cap_rp,
                                                         int64_t cap_nnz,
                                                         int64_t* __restrict__ row_ptr,
                                                         int32_t* __restrict__ hdr) {
  __shared__ uint32_t lds_scan[kTpWaves + 1];
  uint32_t tok = 0, lab = 0, has = 0, tabs = 0, anom = 0;
  for (int64_t c = 0; c < nb; c += kTpBlk) {
    const int64_t i = c + threadIdx.x;
    const bool on = i < nb;
    const int32_t* s = sum + (on ? i : 0) * S_WORDS;
    const uint32_t ntok = on ? (uint32_t)s[S_NTOK] : 0u, lab1 = on ? (uint32_t)s[S_LAB1] : 0u;
    const uint32_t amb = on ? (uint32_t)s[S_AMB] : 0u;
    const uint32_t fn = on ? ((uint32_t)s[S_FN] & 3u) : LineFn::ident;
    const uint32_t tb = on ? (uint32_t)s[S_TAB] : 0u;
    const int an = on ? s[S_ANOM] : 0;
    uint32_t fn_tot, tok_tot, lab_tot, tb_tot;
    const uint32_t fn_ex = tp_block_scan<LineFn>(fn, lds_scan, &fn_tot);
    const uint32_t has_in = (fn_ex & 1) | ((fn_ex >> 1) & has & 1);
    const uint32_t tok_ex = tp_block_scan<Sum>(ntok, lds_scan, &tok_tot);
    const uint32_t lab_ex =
        tp_block_scan<Sum>(lab1 + ((amb && !has_in) ? 1u : 0u), lds_scan, &lab_tot);
    const uint32_t tb_ex = tp_block_scan<TabSeg>(tb, lds_scan, &tb_tot);
    anom |= __syncthreads_or(an) ? 1u : 0u;
    if (on) {
      int32_t* o = bases + i * B_WORDS;
      o[B_TOK] = (int32_t)(tok + tok_ex);
      o[B_LAB] = (int32_t)(lab + lab_ex);
      o[B_HAS] = (int32_t)has_in;
      o[B_TABS] = (int32_t)((tb_ex >> 31) ? (tb_ex & 0x7fffffffu) : tabs + tb_ex);
    }
    tok += tok_tot;
    lab += lab_tot;
    has = (fn_tot & 1) | ((fn_tot >> 1) & has & 1);
    tabs = (tb_tot >> 31) ? (tb_tot & 0x7fffffffu) : tabs + tb_tot;
  }
  if (threadIdx.x == 0)
    tp_write_header(lab, (int64_t)tok - (int64_t)lab, anom, row0, nnz0, cap_rows, cap_rp, cap_nnz,
                    row_ptr, hdr);
}

template <int kFmt>
__global__ void __launch_bounds__(kTpBlk) tp_emit_kernel(
    const uint8_t* __restrict__ text, int64_t n, const int32_t* __restrict__ bases, int64_t row0,
    int64_t nnz0, int64_t cap_rows, int64_t cap_nnz, float* __restrict__ labels,
    int64_t* __restrict__ row_ptr, uint64_t* __restrict__ keys, float* __restrict__ vals,
    int32_t* __restrict__ hdr) {
  __shared__ __attribute__((aligned(16))) uint8_t lds_text[kTpSpan];
  __shared__ uint32_t lds_scan[kTpWaves + 1];
  if (hdr[H_CAP]) return;  // (uniform: set before this launch)
  const int32_t* bs = bases + (int64_t)blockIdx.x * B_WORDS;
  const int64_t base = (int64_t)blockIdx.x * kTpSpan;
  TpThread t;
  TpBlock b;
  tp_classify<kFmt>(text, n, base, lds_text, lds_scan, (uint32_t)bs[B_HAS], (uint32_t)bs[B_TABS],
                    t, b);
  const int64_t rows = hdr[H_ROWS], nnz = hdr[H_NNZ];
  int64_t T = (int64_t)bs[B_TOK] + t.tok_excl;  // global index of the next token
  int64_t L = (int64_t)bs[B_LAB] + t.lab_excl;  // row starts before it
  int bad = 0, defer = 0, nonunit = 0;
  uint32_t r = t.ts;
  while (r) {
    const int i = __ffs((int)r) - 1;
    r &= r - 1;
    const int off = threadIdx.x * kTpBytes + i;
    const int64_t g = base + off;
    const bool is_lab = (t.lab >> i) & 1u;
    if (is_lab) ++L;
    const int64_t R = L - 1;              // this token's row
    const int64_t pos = T - L;            // a feature token's index among the features
    ++T;
    int lim;
    const uint8_t* p = tp_token_window(text, n, base, off, lds_text, &lim);
    int len = 0, colon = -1;
    for (; len < lim; ++len) {
      const uint32_t c = p[len];
      if (c == '\n' || c == '\t') break;
      if (kFmt == kFmtLibsvm || kFmt == kFmtModel) {
        if (c == ' ' || c == '\r') break;
        if (c == ':' && colon < 0) colon = len;
      }
    }
    int st = textnum::kOk;
    if (len > textnum::kMaxTok || R < 0 || R >= rows) {
      st = textnum::kDefer;
    } else if (kFmt == kFmtLibsvm) {
      if (is_lab) {
        float y = 0.f;
        st = p[0] == '#' ? (int)textnum::kDefer : textnum::scan_f32(p, len, &y);
        if (st == textnum::kOk && in_range(row0 + R, cap_rows)) {
          labels[row0 + R] = y;
          row_ptr[row0 + R] = nnz0 + (T - 1 - R);
        }
      } else {
        uint64_t idx = 0;
        float v = 1.f;
        if (colon < 0) {
          st = textnum::kBad;
        } else {
          st = textnum::scan_u64(p, colon, &idx);
          if (st == textnum::kOk && !(len - colon == 2 && p[colon + 1] == '1'))
            st = textnum::scan_f32(p + colon + 1, len - colon - 1, &v);
        }
        if (st == textnum::kOk && pos >= 0 && pos < nnz && in_range(nnz0 + pos, cap_nnz)) {
          keys[nnz0 + pos] = idx;  // (raw: tp_finish compares, tp_mod reduces)
          vals[nnz0 + pos] = v;
          if (v != 1.f) nonunit = 1;
        }
      }
    } else if (kFmt == kFmtModel) {
      // A plain line is digits, one tab, a weight, then '\n' or the end of the text; all of
      // it is decided per token from the bytes next to it. A key must open its line and be
      // followed by a tab and the first byte of a token; a weight must follow a tab and end
      // its line. A weight that ends its line is the line's last token and a key has one
      // right behind it, so when every token passes, every row is one key and one weight
      // and the weight of row R is feature R.
      const auto byte_at = [&](int64_t gg) -> uint32_t {
        if (gg < 0 || gg >= n) return '\n';
        const int64_t q = gg - base;
        return (q >= 0 && q < kTpSpan) ? lds_text[q] : text[gg];
      };
      const uint32_t before = byte_at(g - 1), after = byte_at(g + len);
      if (is_lab) {
        const uint32_t nx = byte_at(g + len + 1);
        uint64_t k = 0;
        if (before != '\n' || after != '\t' || nx == '\n' || nx == '\t' || nx == ' ' ||
            nx == '\r') {
          st = textnum::kDefer;
        } else {
          st = textnum::scan_u64(p, len, &k);
          if (st == textnum::kOk && in_range(row0 + R, cap_rows)) keys[row0 + R] = k;
        }
      } else {
        float v = 0.f;
        // (the scanner takes "+-5"; Python's float takes "+5" and not "+-5": the host decides)
        if (before != '\t' || after != '\n' || p[0] == '+') {
          st = textnum::kDefer;
        } else {
          st = textnum::scan_f32(p, len, &v);
          if (st == textnum::kOk && in_range(row0 + R, cap_rows)) vals[row0 + R] = v;
        }
      }
      if (st == textnum::kBad) st = textnum::kDefer;  // (Python takes "1_0" and "nan")
    } else {
      while (len > 0 && (p[len - 1] == ' ' || p[len - 1] == '\r')) --len;  // (trailing blanks)
      const uint32_t below = (1u << i) - 1u;
      uint32_t field;
      if (t.nl & below) {
        const int top = 31 - __clz((int)(t.nl & below));
        field = (uint32_t)__popc((t.tab & below) >> (top + 1));
      } else {
        field = t.tabs_in + (uint32_t)__popc(t.tab & below);
      }
      if (is_lab) {
        int64_t c = 0;
        // (an empty label field is a bad line; a '#' line is a comment: the host decides)
        st = (field != 0 || p[0] == '#') ? (int)textnum::kDefer : textnum::scan_i64(p, len, &c);
        if (st == textnum::kOk && in_range(row0 + R, cap_rows)) {
          labels[row0 + R] = c > 0 ? 1.f : -1.f;
          row_ptr[row0 + R] = nnz0 + (T - 1 - R);
        }
      } else if (field == 0 || field >= 40) {
        st = textnum::kDefer;  // (fields past the 39th are ignored by the host parser)
      } else {
        const uint32_t j = field - 1;  // slot 0..38
        uint64_t id = 0;
        if (j < 13) {
          int64_t v = 0;
          st = textnum::scan_i64(p, len, &v);
          if (st == textnum::kOk) st = textnum::criteo_bucket(v, &id);
        } else {
          st = textnum::scan_hex(p, len, &id);
        }
        if (st == textnum::kOk && pos >= 0 && pos < nnz && in_range(nnz0 + pos, cap_nnz))
          keys[nnz0 + pos] = textnum::fmix(((uint64_t)(j + 1) << 48) ^ id);
      }
    }
    bad += st == textnum::kBad;
    defer += st == textnum::kDefer;
  }
  tp_report(bad, defer, nonunit, hdr);
}

template <int kFmt>
void tp_launch(const uint8_t* text, int64_t n, uint64_t hash_mod, const TextOut& o, int32_t* work,
               hipStream_t st) {
  const int64_t nb = (n + kTpSpan - 1) / kTpSpan;
  int32_t* sum = work;
  int32_t* bases = work + nb * S_WORDS;
  tp_count_kernel<kFmt><<<(unsigned)nb, kTpBlk, 0, st>>>(text, n, sum);
  tp_scan_kernel<<<1, kTpBlk, 0, st>>>(sum, bases, nb, o.row0, o.nnz0, o.cap_rows, o.cap_rp,
                                    o.cap_nnz, o.row_ptr, o.hdr);
  tp_emit_kernel<kFmt><<<(unsigned)nb, kTpBlk, 0, st>>>(text, n, bases, o.row0, o.nnz0, o.cap_rows,
                                                       o.cap_nnz, o.labels, o.row_ptr, o.keys,
                                                       o.vals, o.hdr);
  tp_finish(o, n, kFmt == kFmtLibsvm, hash_mod, st);
}

// The kernel family of a text format (the .hip file with its kernels); throws for a format
// without a device parser.
enum { kFamTp, kFamPs, kFamAd };
int family_of(int fmt) {
  switch (fmt) {
    case kFmtLibsvm: case kFmtCriteo: return kFamTp;
    case kFmtSparse: case kFmtSparseBinary: return kFamPs;
    case kFmtAdfea: case kFmtTerafea: return kFamAd;
  }
  throw std::invalid_argument("textparse: no device parser for this text format");
}

}  // namespace

int64_t textparse_span() { return kTpSpan; }
int64_t textparse_work_words(int64_t n, int fmt) {
  switch (family_of(fmt)) {
    case kFamTp: return ((n + kTpSpan - 1) / kTpSpan) * (S_WORDS + B_WORDS) + 16;
    case kFamPs: return ps_work_words(n);
    default: return ad_work_words(n);
  }
}

// The one entry of the six device parsers: the argument checks, then the format's launcher
// (here, pstext.hip, adtext.hip).
void textparse(const uint8_t* text, int64_t n, int fmt, uint64_t hash_mod, const TextOut& out,
               int32_t* work, hipStream_t st) {
  const int family = family_of(fmt);
  if (n <= 0 || n > ((int64_t)1 << 30))
    throw std::invalid_argument("textparse: chunk size must be in [1, 2^30] bytes");
  if (((uintptr_t)text & 15) != 0)
    throw std::invalid_argument("textparse: text buffer must be 16-byte aligned");
  if ((fmt == kFmtLibsvm || fmt == kFmtSparse) && !out.vals)
    throw std::invalid_argument("textparse: LIBSVM and SPARSE need vals");
  if (family == kFamPs) return ps_launch(text, n, fmt == kFmtSparse, hash_mod, out, work, st);
  if (family == kFamAd) return ad_launch(text, n, fmt == kFmtAdfea, hash_mod, out, work, st);
  if (fmt == kFmtLibsvm) return tp_launch<kFmtLibsvm>(text, n, hash_mod, out, work, st);
  return tp_launch<kFmtCriteo>(text, n, hash_mod, out, work, st);
}

// key<TAB>weight model text (utils/checkpoint.py): keys[r] / w[r] of line r, in file order.
// The chunk counts only if hdr reports no H_CAP / H_BAD / H_DEFER and H_ROWS == H_NNZ; else
// the caller parses it by the host rules. text: n bytes, 16-byte aligned, starting at a line
// start. hdr / work as for textparse.
void modeltext_parse(const uint8_t* text, int64_t n, uint64_t* keys, float* w, int64_t cap,
                     int32_t* hdr, int32_t* work, hipStream_t st) {
  if (n <= 0 || n > ((int64_t)1 << 30))
    throw std::invalid_argument("modeltext_parse: chunk size must be in [1, 2^30] bytes");
  if (((uintptr_t)text & 15) != 0)
    throw std::invalid_argument("modeltext_parse: text buffer must be 16-byte aligned");
  const int64_t nb = (n + kTpSpan - 1) / kTpSpan;
  int32_t* sum = work;
  int32_t* bases = work + nb * S_WORDS;
  tp_count_kernel<kFmtModel><<<(unsigned)nb, kTpBlk, 0, st>>>(text, n, sum);
  tp_scan_kernel<<<1, kTpBlk, 0, st>>>(sum, bases, nb, 0, 0, cap, cap + 1, cap, nullptr, hdr);
  tp_emit_kernel<kFmtModel><<<(unsigned)nb, kTpBlk, 0, st>>>(text, n, bases, 0, 0, cap, cap,
                                                            nullptr, nullptr, keys, w, hdr);
  PSAMD_HIP_CHECK(hipGetLastError());
}

// row_ptr[i] -= delta for i < n (a minibatch's offsets out of a chunk's).
__global__ void __launch_bounds__(256) tp_rebase_kernel(const int64_t* __restrict__ in,
                                                        int64_t* __restrict__ out, int64_t n,
                                                        int64_t delta) {
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n;
       i += (int64_t)gridDim.x * blockDim.x)
    out[i] = in[i] - delta;
}

void textparse_rebase(const int64_t* in, int64_t* out, int64_t n, int64_t delta, hipStream_t st) {
  if (n <= 0) return;
  tp_rebase_kernel<<<grid_for(n, 256, 1024), 256, 0, st>>>(in, out, n, delta);
  PSAMD_HIP_CHECK(hipGetLastError());
}

// flags[s] = any vals[j] != 1 for j in [bounds[s], bounds[s + 1]): which minibatches cut out
// of a parsed chunk carry values (all-ones values are binary features). One workgroup per
// segment; bounds are clamped to the value buffer.
__global__ void __launch_bounds__(256) tp_seg_nonunit_kernel(const float* __restrict__ vals,
                                                             int64_t cap,
                                                             const int64_t* __restrict__ bounds,
                                                             int nseg, int32_t* __restrict__ flags) {
  for (int s = blockIdx.x; s < nseg; s += gridDim.x) {
    int64_t a = bounds[s], b = bounds[s + 1];
    a = a < 0 ? 0 : a;
    b = b > cap ? cap : b;
    int any = 0;
    for (int64_t j = a + threadIdx.x; j < b; j += blockDim.x) any |= vals[j] != 1.f;
    any = __syncthreads_or(any);
    if (threadIdx.x == 0) flags[s] = any ? 1 : 0;
  }
}

void textparse_seg_nonunit(const float* vals, int64_t cap, const int64_t* bounds, int nseg,
                           int32_t* flags, hipStream_t st) {
  if (nseg <= 0) return;
  tp_seg_nonunit_kernel<<<nseg < 4096 ? nseg : 4096, 256, 0, st>>>(vals, cap, bounds, nseg, flags);
  PSAMD_HIP_CHECK(hipGetLastError());
}

}  // namespace psamd
