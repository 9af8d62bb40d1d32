// Host entry point of fwfm_predict.hip: score a minibatch of raw keys against a slot table
// and the factor rows at the slot index of every key, read as a field-weighted factorization
// machine (one vector of D bf16 per key, field-pair strengths R [F, F]).
#pragma once
#include <hip/hip_runtime.h>
#include <cstdint>

#include "common.cuh"
#include "params.h"

namespace psamd {

// The contract of ffm_predict_rows (ffm_predict.h) with the FwFM's geometry: rows [t.cap, D]
// bf16 with D in {8, 16, 32}, F in 1..64, R [F, F] f32 on the device, read as symmetric from
// its upper triangle (the diagonal acts in a row where its field occurs at least twice). With
// row_ptr, fields [nnz] int32 names the field of every occurrence; with a fixed width,
// field_of [field_of_len == width] int32 maps position -> field (null: the position is the
// field). A field outside [0, F) keeps the occurrence's linear term and takes it out of every
// pair. t.cap <= 2^31, nnz < 2^31, rows 16-byte aligned. Anything else throws
// std::invalid_argument before a launch; B == 0 launches nothing.
void fwfm_predict_rows(const TableRef& t, KeyMix km, const void* rows, int D, int F,
                       const float* R, const uint64_t* keys, int64_t nnz, const int64_t* row_ptr,
                       int width, const int32_t* fields, const int32_t* field_of,
                       int64_t field_of_len, const float* vals, const float* labels, int64_t B,
                       int loss_type, float* margin, const StripedAcc& metrics,
                       unsigned long long* hist, int nbins, int hist_stripes, hipStream_t st);

}  // namespace psamd
