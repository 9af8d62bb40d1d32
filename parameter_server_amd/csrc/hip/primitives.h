// Host entry points of primitives.hip: radix sort of (u64 key, i32 value) pairs and the
// i32 scan. temp: scratch of >= the matching *_temp_bytes(n).
#pragma once
#include <hip/hip_runtime.h>
#include <cstddef>
#include <cstdint>

namespace psamd {

size_t radix_sort_temp_bytes(int64_t n);
// sorts on key bits [0, end_bit); inputs and outputs must not alias
void radix_sort_pairs(void* temp, size_t temp_bytes, const uint64_t* k_in, uint64_t* k_out,
                      const int32_t* v_in, int32_t* v_out, int64_t n, int end_bit,
                      hipStream_t st);
size_t scan_i32_temp_bytes(int64_t n);
void scan_i32(const int32_t* in, int32_t* out, int64_t n, void* temp, bool inclusive,
              hipStream_t st);

}  // namespace psamd
