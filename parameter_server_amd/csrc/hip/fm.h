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

}  // namespace psamd
