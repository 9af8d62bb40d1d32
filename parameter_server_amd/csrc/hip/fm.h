// Host entry points of fm.hip: the factorization machine's fused forward / backward.
#pragma once
#include <hip/hip_runtime.h>
#include <cstdint>

namespace psamd {

// X0 ([B * S, D] bf16, expanded) or rows ([rows_cap, D] bf16 read through local_col and
// idx, which may be null): exactly one is non-null. vals, hist may be null.
void fm_fwd_bwd(const void* X0, const void* rows, const int64_t* idx, int64_t idx_cap,
                int64_t rows_cap, const float* vals, int64_t B, int S, int D,
                const int32_t* local_col, const float* w_local, int64_t w_cap, const float* labels,
                float* coef, void* dX0, double* metrics, uint32_t* hist, int nbins,
                int acc_stripes, hipStream_t st);
// dE += lambda * rows (through idx when given); n_dev may be null
void fm_l2(float* dE, const void* rows, const int64_t* idx, int64_t rows_cap, const int32_t* n_dev,
           int64_t u_cap, int D, float lambda, hipStream_t st);

// fm_csr: the same forward / backward on CSR rows of any width (fm.hip, lane groups).
// Row b holds positions [row_ptr[b], row_ptr[b + 1]), or [b * width, + width) when
// row_ptr is null; both ends are clamped to nnz. local_col may be null (column =
// position: per-occurrence idx / w_local, as scoring resolves them). Factor rows are read
// as rows[idx ? idx[col] : col]; idx[col] == -1 or an index out of range is a zero row.
struct FmCsr {
  const int64_t* row_ptr;
  int width;
  int64_t nnz, B;
  const int32_t* local_col;
  const float* vals;
  const void* rows;  // [rows_cap, D] bf16
  const int64_t* idx;
  int64_t idx_cap, rows_cap;
  const float* w_local;
  int64_t w_cap;
  int D;
  // training form (fm_csr): everything below but margins; forward-only form
  // (fm_csr_margins): margins alone
  const float* labels;
  float* coef;      // [B]
  void* dX0;        // [nnz, D] bf16
  int32_t* row_of;  // [nnz] row id of every occurrence
  double* metrics;
  uint32_t* hist;   // may be null
  int nbins, acc_stripes;
  float* margins;   // [B]
};
// lanes per row from the mean width nnz / B: 16, 32 or 64
int fm_csr_lanes(int64_t nnz, int64_t B);
// lanes: 0 = fm_csr_lanes, else 16, 32 or 64; D in {8, 16, 32}, anything else throws
void fm_csr(const FmCsr& a, int lanes, hipStream_t st);
void fm_csr_margins(const FmCsr& a, int lanes, hipStream_t st);

}  // namespace psamd
