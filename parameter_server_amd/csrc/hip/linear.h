// Host entry points of linear.hip: the linear model's forward / backward, the AUC
// reduction and the synthetic Criteo generator.
#pragma once
#include <hip/hip_runtime.h>
#include <cstdint>

#include "params.h"

namespace psamd {

// row_ptr null: fixed row width. vals, xw, coef2, metrics (>= 5 striped slots), hist
// (hist_stripes x 2 x nbins) may be null; w_cap: capacity of w_local
void linear_fwd(const int64_t* row_ptr, int64_t B, int width, const int32_t* local_col,
                const float* vals, const float* w_local, int64_t w_cap, const float* labels,
                int loss_type, float* xw, float* coef, float* coef2, double* metrics,
                uint32_t* hist, int nbins, int acc_stripes, int hist_stripes, hipStream_t st);
// rows null: fixed row width; vals, coef2, hess may be null; B: capacity of coef
void linear_bwd(const int32_t* pos_s, const int32_t* segid, int64_t n, const int32_t* rows,
                int width, const float* vals, const float* coef, int64_t B, const float* coef2,
                float* grad, float* hess, int64_t grad_cap, hipStream_t st);
// auc.hist required, 2048 bins, <= 8 stripes; step_counter may be null
void auc_from_hist(const AucOut& auc, hipStream_t st);
// rows[i] = row of occurrence i, for row_ptr [B + 1]
void csr_rows(const int64_t* row_ptr, int64_t B, int32_t* rows, hipStream_t st);
// host arrays: 26 cardinalities, 256 Gaussian quantiles (copied to constant memory)
void criteo_set_tables(const uint32_t* cards26, const float* gauss256);
// rows [row0 (+ *row0_dev * row_scale), + B); row0_dev / row0_out may be null (row0_out
// receives *row0_dev + 1)
void criteo_gen(uint64_t seed, int64_t row0, const int64_t* row0_dev, int64_t row_scale,
                int64_t B, uint64_t num_features, float alpha, uint64_t* keys, float* labels,
                int64_t* row0_out, hipStream_t st);
void add_i64(int64_t* p, int64_t v, hipStream_t st);

}  // namespace psamd
