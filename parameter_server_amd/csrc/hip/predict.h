// Host entry point of predict.hip: score a minibatch of raw keys against a slot table.
#pragma once
#include <hip/hip_runtime.h>
#include <cstdint>

#include "common.cuh"
#include "params.h"

namespace psamd {

// row_ptr null: fixed row width. vals, labels, margin, metrics.ptr ([loss, correct,
// count] sums), hist (u64 stripes x 2 x nbins) may be null; metrics / hist need labels.
// lanes per row: 0 = from nnz / B, else 8 or 64.
void predict_rows(const TableRef& t, KeyMix km, const uint64_t* keys, int64_t nnz,
                  const int64_t* row_ptr, int width, const float* vals, const float* labels,
                  int64_t B, int loss_type, float* margin, const StripedAcc& metrics,
                  unsigned long long* hist, int nbins, int hist_stripes, int lanes,
                  hipStream_t st);

}  // namespace psamd
