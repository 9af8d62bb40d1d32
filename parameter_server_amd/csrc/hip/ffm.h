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

}  // namespace psamd
