// Host entry points of fwfm.hip: the field-weighted factorization machine's fused forward /
// backward on rows of a fixed width S <= 64, and the fixed-order reduction of its dR partials;
// of fwfm_csr.hip: the same on CSR rows of any width with a field per occurrence.
#pragma once
#include <hip/hip_runtime.h>
#include <cstdint>

namespace psamd {

// Position i of a row has field fields[i] in [0, F) (one map for all rows). A key's table
// row is one vector of Dr = D bf16 (the FM's row); R [F, F] fp32 holds the field-pair
// strengths and is read as symmetric: R[min(f, g)][max(f, g)], the lower triangle is never
// read; R[f][f] of a field with fewer than two positions (no same-field pair) is read as 0
// and its gradient is 0. Factor rows are read as rows[idx ? idx[col] : col] with col =
// local_col ? local_col[p] : p; idx[col] == -1 or an index out of range is a zero row, a
// column out of range a zero weight and a zero row (as Ffm).
struct Fwfm {
  int64_t B;
  int S, F, Dr;           // Dr: the factor dimension D, named as Ffm's row width
  const int32_t* fields;  // [S], HOST memory: the launcher packs it into the kernel argument
  const int32_t* local_col;
  const float* vals;
  const void* rows;  // [rows_cap, Dr] bf16
  const int64_t* idx;
  int64_t idx_cap, rows_cap;
  const float* w_local;
  int64_t w_cap;
  const float* R;  // [F, F], DEVICE memory
  // training form (fwfm_fwd_bwd): everything below but margins; forward-only form
  // (fwfm_margins): margins alone
  const float* labels;
  float* coef;      // [B]
  void* dX0;        // [B * S, Dr] bf16
  float* dR_part;   // [parts, Fp * Fp], Fp = F rounded up to 16: one partial per block; the
  int parts;        // launch has exactly `parts` blocks, and every one writes its partial
  double* metrics;
  uint32_t* hist;   // may be null
  int nbins, acc_stripes;
  float* margins;   // [B]
};
// S in 1..64, F in 1..64, Dr in {8, 16, 32}, every field in [0, F), parts in 1..4096:
// anything else throws std::invalid_argument before a launch.
void fwfm_fwd_bwd(const Fwfm& a, hipStream_t st);
void fwfm_margins(const Fwfm& a, hipStream_t st);

// dR [F, F] (symmetric) from the partials of fwfm_fwd_bwd, summed in a fixed order (16 runs
// of consecutive blocks, then the 16 runs), and / or the AdaGrad step of R on it:
//   g = dR + lambda_r R;  acc += g^2;  R -= lr g / (sqrt(acc) + 1e-8)
// sum && update: one rank. sum alone, an all-reduce of dR, update alone: several.
struct FwfmReduce {
  int F, parts;
  const float* dR_part;  // [parts, Fp * Fp]; read when sum
  float* dR;             // [F, F]: written when sum, read when !sum
  bool sum, update;
  float* R;              // [F, F], with update
  float* acc;            // [F, F], with update
  float lr, lambda_r;
};
void fwfm_dr_reduce(const FwfmReduce& a, hipStream_t st);

// fwfm_csr.hip: the same model on CSR rows of any width with a field per occurrence. Row b
// holds positions [row_ptr[b], row_ptr[b + 1]), both ends clamped to nnz; occurrence p has
// field fld[p]. A field outside [0, F) keeps the occurrence's linear term and takes it out of
// every pair (its dX0 row is zero). R[f][f] acts in a row where field f occurs at least
// twice, and there only: elsewhere it adds exactly 0 to the margin, dX0 and dR[f][f]. Rows,
// idx, local_col, w_local and R as Fwfm; dR_part as Fwfm's, for fwfm_dr_reduce.
struct FwfmCsr {
  const int64_t* row_ptr;  // [B + 1]
  int64_t B, nnz;
  int F, Dr;
  const int32_t* fld;      // [nnz], DEVICE memory
  const int32_t* local_col;
  const float* vals;
  const void* rows;  // [rows_cap, Dr] bf16
  const int64_t* idx;
  int64_t idx_cap, rows_cap;
  const float* w_local;
  int64_t w_cap;
  const float* R;  // [F, F], DEVICE memory
  // training form (fwfm_csr_fwd_bwd): everything below but margins; forward-only form
  // (fwfm_csr_margins): margins alone
  const float* labels;
  float* coef;      // [B]
  void* dX0;        // [nnz, Dr] bf16
  int32_t* row_of;  // [nnz] row id of every occurrence
  float* dR_part;   // [parts, Fp * Fp]: the launch has exactly `parts` blocks
  int parts;
  double* metrics;
  uint32_t* hist;   // may be null
  int nbins, acc_stripes;
  float* margins;   // [B]
};
// F in 1..64, Dr in {8, 16, 32}, nnz < 2^31, parts in 1..4096: anything else throws
// std::invalid_argument before a launch.
void fwfm_csr_fwd_bwd(const FwfmCsr& a, hipStream_t st);
void fwfm_csr_margins(const FwfmCsr& a, hipStream_t st);

}  // namespace psamd
