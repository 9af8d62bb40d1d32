// Host entry points of ffm.hip: the field-aware factorization machine's fused forward /
// backward on rows of a fixed width S <= 64.
#pragma once
#include <hip/hip_runtime.h>
#include <cstdint>

namespace psamd {

// Position i of a row has field fields[i] in [0, F) (one map for all rows). A key's table
// row holds F vectors of k bf16, v_{i,f} = row_i[f * k, + k), in a row of Dr >= F * k
// columns (Dr % 8 == 0, the columns past F * k are never read and their gradient is 0).
// Factor rows are read as rows[idx ? idx[col] : col] with col = local_col ? local_col[p] : p;
// idx[col] == -1 or an index out of range is a zero row, a column out of range a zero
// weight and a zero row (as fm_csr_load).
struct Ffm {
  int64_t B;
  int S, F, k, Dr;
  const int32_t* fields;  // [S], HOST memory: the launcher packs it into the kernel argument
  const int32_t* local_col;
  const float* vals;
  const void* rows;  // [rows_cap, Dr] bf16
  const int64_t* idx;
  int64_t idx_cap, rows_cap;
  const float* w_local;
  int64_t w_cap;
  // training form (ffm_fwd_bwd): everything below but margins; forward-only form
  // (ffm_margins): margins alone
  const float* labels;
  float* coef;      // [B]
  void* dX0;        // [B * S, Dr] bf16
  double* metrics;
  uint32_t* hist;   // may be null
  int nbins, acc_stripes;
  float* margins;   // [B]
};
// S in 1..64, k in {2, 4, 8}, F * k <= Dr <= 128, Dr % 8 == 0, every field in [0, F):
// anything else throws std::invalid_argument before a launch.
void ffm_fwd_bwd(const Ffm& a, hipStream_t st);
void ffm_margins(const Ffm& a, hipStream_t st);

// ffm_csr.hip: the same model on CSR rows with a field per occurrence. Row b holds positions
// [row_ptr[b], row_ptr[b + 1]), both ends clamped to nnz; occurrence p has field fld[p]. A
// field outside [0, F) keeps the occurrence's linear term and takes it out of every pair
// (its dX0 row is zero). Rows of up to T positions run on a per-wave LDS tile, wider rows
// (any width) on a second launch that reads partners from global memory. Rows, idx, local_col
// and w_local as Ffm.
struct FfmCsr {
  const int64_t* row_ptr;  // [B + 1]
  int64_t B, nnz;
  int T, F, k, Dr;         // T: the tile's row capacity
  const int32_t* fld;      // [nnz], DEVICE memory
  const int32_t* local_col;
  const float* vals;
  const void* rows;  // [rows_cap, Dr] bf16
  const int64_t* idx;
  int64_t idx_cap, rows_cap;
  const float* w_local;
  int64_t w_cap;
  // training form (ffm_csr): everything below but margins; forward-only form
  // (ffm_csr_margins): margins alone
  const float* labels;
  float* coef;      // [B]
  void* dX0;        // [nnz, Dr] bf16
  int32_t* row_of;  // [nnz] row id of every occurrence
  double* metrics;
  uint32_t* hist;   // may be null
  int nbins, acc_stripes;
  float* margins;   // [B]
};
// T in 1..64, k in {2, 4, 8}, F * k <= Dr <= 128, Dr % 8 == 0, nnz < 2^31: anything else
// throws std::invalid_argument before a launch.
void ffm_csr(const FfmCsr& a, hipStream_t st);
void ffm_csr_margins(const FfmCsr& a, hipStream_t st);

}  // namespace psamd
