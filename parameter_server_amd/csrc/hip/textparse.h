// Host entry points of textparse.hip: LIBSVM / Criteo text and key<TAB>weight model text
// parsed on the GPU. hdr: 8 result words; work: >= textparse_work_words(n) words.
#pragma once
#include <hip/hip_runtime.h>
#include <cstdint>

namespace psamd {

int64_t textparse_span();  // (no caller left: bytes of text one workgroup scans)
int64_t textparse_work_words(int64_t n);
// n bytes of text; rows from row0, entries from nnz0; cap_*: capacities of labels,
// row_ptr and keys / vals; vals may be null
void textparse(const uint8_t* text, int64_t n, int fmt, uint64_t hash_mod, int64_t row0,
               int64_t nnz0, float* labels, int64_t cap_rows, int64_t* row_ptr, int64_t cap_rp,
               uint64_t* keys, float* vals, int64_t cap_nnz, int32_t* hdr, int32_t* work,
               hipStream_t st);
// cap: capacity of keys / w
void modeltext_parse(const uint8_t* text, int64_t n, uint64_t* keys, float* w, int64_t cap,
                     int32_t* hdr, int32_t* work, hipStream_t st);
// out[i] = in[i] + delta
void textparse_rebase(const int64_t* in, int64_t* out, int64_t n, int64_t delta, hipStream_t st);
// flags[s] = segment [bounds[s], bounds[s + 1]) holds a value != 1; cap: capacity of vals
void textparse_seg_nonunit(const float* vals, int64_t cap, const int64_t* bounds, int nseg,
                           int32_t* flags, hipStream_t st);

}  // namespace psamd
