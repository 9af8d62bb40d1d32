// Host entry point of ffm_predict.hip: score a minibatch of raw keys against a slot table
// and the factor rows at the slot index of every key, read as a field-aware factorization
// machine (F fields of k bf16 in a row of Dr columns).
#pragma once
#include <hip/hip_runtime.h>
#include <cstdint>

#include "common.cuh"
#include "params.h"

namespace psamd {

// The contract of fm_predict_rows (fm_predict.h) plus the fields: with row_ptr, fields [nnz]
// int32 names the field of every occurrence; with a fixed width, field_of [field_of_len ==
// width] int32 maps position -> field (null: the position is the field). A field outside
// [0, F) keeps the occurrence's linear term and takes it out of every pair. k in {2, 4, 8},
// F k <= Dr <= 128, Dr % 8 == 0, t.cap <= 2^31, nnz < 2^31, rows 16-byte aligned. Anything
// else throws std::invalid_argument before a launch.
void ffm_predict_rows(const TableRef& t, KeyMix km, const void* rows, int Dr, int F, int k,
                      const uint64_t* keys, int64_t nnz, const int64_t* row_ptr, int width,
                      const int32_t* fields, const int32_t* field_of, int64_t field_of_len,
                      const float* vals, const float* labels, int64_t B, int loss_type,
                      float* margin, const StripedAcc& metrics, unsigned long long* hist,
                      int nbins, int hist_stripes, hipStream_t st);

}  // namespace psamd
