// Host entry points of pstext.hip: the slot-grouped text formats SPARSE_BINARY / SPARSE
// ("label; grp key ...; grp key:val ...;") parsed on the GPU. hdr: the 8 result words of
// textparse.h; work: >= pstext_work_words(n) words.
#pragma once
#include <hip/hip_runtime.h>
#include <cstdint>

namespace psamd {

int64_t pstext_work_words(int64_t n);
// n bytes of text; rows from row0, entries from nnz0; cap_*: capacities of labels, row_ptr
// and keys / vals / slots. vals may be null for SPARSE_BINARY. slots null: group heads are
// not read (ignore_slot); else every entry gets its group head's value.
void pstext(const uint8_t* text, int64_t n, int fmt, uint64_t hash_mod, int64_t row0,
            int64_t nnz0, float* labels, int64_t cap_rows, int64_t* row_ptr, int64_t cap_rp,
            uint64_t* keys, float* vals, int32_t* slots, int64_t cap_nnz, int32_t* hdr,
            int32_t* work, hipStream_t st);

}  // namespace psamd
