// Host entry points of adtext.hip: the CTR log formats ADFEA ("lineid 1 click key:grp ...")
// and TERAFEA ("click lineid | key key ...") parsed on the GPU. hdr: the 8 result words of
// textparse.h; work: >= adtext_work_words(n) words.
#pragma once
#include <hip/hip_runtime.h>
#include <cstdint>

namespace psamd {

int64_t adtext_work_words(int64_t n);
// n bytes of text; rows from row0, entries from nnz0; cap_*: capacities of labels, row_ptr
// and keys / slots. Both formats are binary: there are no values. slots null: every entry's
// group is 1 on the host (ignore_slot) and nothing is written, ADFEA group tokens are not
// validated; else ADFEA entries get their group token, TERAFEA entries key >> 54.
void adtext(const uint8_t* text, int64_t n, int fmt, uint64_t hash_mod, int64_t row0,
            int64_t nnz0, float* labels, int64_t cap_rows, int64_t* row_ptr, int64_t cap_rp,
            uint64_t* keys, int32_t* slots, int64_t cap_nnz, int32_t* hdr, int32_t* work,
            hipStream_t st);

}  // namespace psamd
