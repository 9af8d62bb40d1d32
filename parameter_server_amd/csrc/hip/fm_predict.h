// Host entry point of fm_predict.hip: score a minibatch of raw keys against a slot table
// and the factor rows that sit at the slot index of every key (the factorization machine).
#pragma once
#include <hip/hip_runtime.h>
#include <cstdint>

#include "common.cuh"
#include "params.h"

namespace psamd {

// The contract of predict_rows (predict.h) plus rows [t.cap, D] bf16, D a multiple of 8
// up to 128, 16-byte aligned; t.cap <= 2^31. lanes per row: 0 = fm_csr_lanes(nnz, B),
// else 16, 32 or 64. Anything else throws before a launch.
void fm_predict_rows(const TableRef& t, KeyMix km, const void* rows, int D, const uint64_t* keys,
                     int64_t nnz, const int64_t* row_ptr, int width, const float* vals,
                     const float* labels, int64_t B, int loss_type, float* margin,
                     const StripedAcc& metrics, unsigned long long* hist, int nbins,
                     int hist_stripes, int lanes, hipStream_t st);

}  // namespace psamd
