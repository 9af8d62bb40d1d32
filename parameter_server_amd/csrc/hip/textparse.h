// Host entry points of the device text parsers: LIBSVM / CRITEO (textparse.hip), the
// slot-grouped SPARSE / SPARSE_BINARY ("label; grp key ...; grp key:val ...;", pstext.hip)
// and the CTR logs ADFEA ("lineid 1 click key:grp ...") / TERAFEA ("click lineid | key key
// ...", adtext.hip) behind one textparse(), and key<TAB>weight model text. hdr: 8 result
// words; work: >= textparse_work_words(n, fmt) words.
#pragma once
#include <hip/hip_runtime.h>
#include <cstdint>

namespace psamd {

constexpr int kFmtLibsvm = 5, kFmtCriteo = 8, kFmtSparse = 2, kFmtSparseBinary = 3,
              kFmtAdfea = 4, kFmtTerafea = 6;  // data.TEXT_FORMATS

// Where a parsed chunk goes: rows from row0, entries from nnz0; cap_*: capacities of labels,
// row_ptr and keys / vals / slots. vals: null unless the format carries values (LIBSVM,
// SPARSE). slots null: groups are not read (ignore_slot; LIBSVM and CRITEO have none); else
// every entry gets its group (SPARSE*: its group head's value, ADFEA: its group token,
// TERAFEA: key >> 54).
struct TextOut {
  float* labels;
  int64_t cap_rows;
  int64_t* row_ptr;
  int64_t cap_rp;
  uint64_t* keys;
  float* vals;
  int32_t* slots;
  int64_t cap_nnz;
  int64_t row0, nnz0;
  int32_t* hdr;
};

int64_t textparse_span();  // (no caller left: bytes of text one workgroup scans)
int64_t textparse_work_words(int64_t n, int fmt = kFmtLibsvm);
// n bytes of fmt text, 16-byte aligned, into out; hdr's H_CAP must be cleared by the caller
// before the first use
void textparse(const uint8_t* text, int64_t n, int fmt, uint64_t hash_mod, const TextOut& out,
               int32_t* work, hipStream_t st);
// cap: capacity of keys / w
void modeltext_parse(const uint8_t* text, int64_t n, uint64_t* keys, float* w, int64_t cap,
                     int32_t* hdr, int32_t* work, hipStream_t st);
// out[i] = in[i] + delta
void textparse_rebase(const int64_t* in, int64_t* out, int64_t n, int64_t delta, hipStream_t st);
// flags[s] = segment [bounds[s], bounds[s + 1]) holds a value != 1; cap: capacity of vals
void textparse_seg_nonunit(const float* vals, int64_t cap, const int64_t* bounds, int nseg,
                           int32_t* flags, hipStream_t st);

// Internal: the launchers of pstext.hip and adtext.hip that textparse() dispatches to, behind
// its argument checks.
int64_t ps_work_words(int64_t n);
void ps_launch(const uint8_t* text, int64_t n, bool valued, uint64_t hash_mod, const TextOut& out,
               int32_t* work, hipStream_t st);
int64_t ad_work_words(int64_t n);
void ad_launch(const uint8_t* text, int64_t n, bool adfea, uint64_t hash_mod, const TextOut& out,
               int32_t* work, hipStream_t st);

}  // namespace psamd
