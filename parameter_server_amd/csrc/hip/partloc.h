// Host entry points of partloc.hip: localisation by bucket partition (key bits <= 32,
// n <= 10 M).
#pragma once
#include <hip/hip_runtime.h>
#include <cstddef>
#include <cstdint>

#include "common.cuh"

namespace psamd {

size_t partloc_temp_bytes(int64_t n, int bits);
bool partloc_supported(int64_t n, int bits);
// zero_a / zero_b (may be null): n floats each to clear; u_cap: capacity of uniq;
// err: set when a bucket overflows
void localize_part(const uint64_t* raw, int64_t n, KeyMix m, void* temp, size_t temp_bytes,
                   int32_t* pos_s, int32_t* segid, uint64_t* uniq, int32_t* seg_start,
                   int32_t* local_col, int32_t* n_uniq, float* zero_a, float* zero_b,
                   int32_t* err, int64_t u_cap, hipStream_t st);

}  // namespace psamd
