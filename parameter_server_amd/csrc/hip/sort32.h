// Host entry points of sort32.hip: fused mix + sort + RLE for keys of <= 32 bits
// (localize32), the 40-bit sort, and their device-count variants.
#pragma once
#include <hip/hip_runtime.h>
#include <cstddef>
#include <cstdint>

#include "common.cuh"

namespace psamd {

size_t localize32_temp_bytes(int64_t n);
// zero_a / zero_b (may be null): n floats each to clear; digit_bits 8 or 10
void localize32(const uint64_t* raw, int64_t n, KeyMix m, void* temp, size_t temp_bytes,
                uint32_t* hs, int32_t* pos_s, int32_t* segid, uint64_t* uniq, int32_t* seg_start,
                int32_t* local_col, int32_t* n_uniq, float* zero_a, float* zero_b, int digit_bits,
                hipStream_t st);
size_t sort40_temp_bytes(int64_t n);
// 30 < key bits <= 40, n < 2^22
void sort40(const uint64_t* raw, int64_t n, KeyMix m, void* temp, size_t temp_bytes,
            uint64_t* hs, int32_t* pos_s, hipStream_t st);
size_t sort32_dev_temp_bytes(int64_t n_max);
// sort + RLE of a device-counted key list (n_dev <= n_max); p_cap: capacity of uniq
void sort_rle32_dev(const uint32_t* keys_in, const int32_t* tile_cnt, int64_t n_max,
                    const int32_t* n_dev, int bits, int digit_bits, void* temp, size_t temp_bytes,
                    uint32_t* hs, int32_t* pos_s, int32_t* segid, uint64_t* uniq,
                    int32_t* seg_start, int32_t* ent_uid, int64_t p_cap, int32_t* n_uniq,
                    float* zero_a, hipStream_t st);

}  // namespace psamd
