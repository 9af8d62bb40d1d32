// Host entry points of slotsplit.hip: one parsed chunk (CSR row_ptr / keys / vals and the
// feature group of every entry, as pstext.hip leaves them) split by feature group on the
// GPU into slot-major keys / vals and one row-offset array per group, what
// SlotData.from_batch makes of the same arrays on the host.
//
// hdr: slotsplit_hdr_words() int32 = 8 result words, the ascending group ids and the
// groups' totals (SS_* below). work: >= slotsplit_work_words(nnz, cells) int32.
//
// A strict fast path: a chunk is left to the host (SS_FLAGS != 0, nothing in the outputs
// is valid) when it names more than slotsplit_max_ids() groups or a group id outside
// [0, 2^31) (kSsIds), when a row names a group twice (kSsRepeat: two runs of one group in
// one row have no order among unordered atomics), or when S * (R + 1) exceeds the cell
// cap (kSsCells). The default cap, slotsplit_default_cell_cap() = 2^24 cells, keeps the
// two int32 cell arrays of the work space at 128 MiB; any cap up to 2^30 may be passed.
#pragma once
#include <hip/hip_runtime.h>
#include <cstdint>

namespace psamd {

enum { SS_S, SS_FLAGS, SS_NCELLS, SS_TOTAL, SS_IDS = 8 };  // totals at SS_IDS + max_ids
enum { kSsIds = 1, kSsRepeat = 2, kSsCells = 4, kSsInput = 8 };  // SS_FLAGS bits

int slotsplit_tile();     // features per workgroup of the per-feature kernels
int slotsplit_max_ids();  // 4096, the reference's kSlotIDmax
int64_t slotsplit_default_cell_cap();
int64_t slotsplit_hdr_words();
int64_t slotsplit_work_words(int64_t nnz, int64_t cells);

// row_ptr [R + 1] (any base: row_ptr[0] is subtracted), keys / vals (null: binary) /
// slots [nnz]; 1 <= R, 1 <= nnz < 2^31. cells: the cell arrays' size in the work space,
// cell_cap <= cells. Writes keys_out / vals_out [nnz] and hdr.
void slotsplit(const int64_t* row_ptr, int64_t R, const uint64_t* keys, const float* vals,
               const int32_t* slots, int64_t nnz, int64_t cell_cap, int64_t cells,
               uint64_t* keys_out, float* vals_out, int32_t* hdr, int32_t* work, hipStream_t st);
// After a clean slotsplit with the same nnz / cells / work: off [S][R + 1] int64, the row
// offsets of every group relative to its own first entry (S read back from hdr).
void slotsplit_offsets(const int32_t* work, int64_t nnz, int64_t cells, int64_t R, int64_t S,
                       int64_t* off, hipStream_t st);

}  // namespace psamd
