// Host entry points of localize.hip: key mixing, run-length encoding of sorted keys and
// the owner split.
#pragma once
#include <hip/hip_runtime.h>
#include <cstddef>
#include <cstdint>

#include "common.cuh"

namespace psamd {

// h[i] = mix(keys[i]), pos[i] = i
void mix_iota(const uint64_t* keys, int64_t n, KeyMix m, uint64_t* h, int32_t* pos,
              hipStream_t st);
void mix_keys(const uint64_t* keys, int64_t n, KeyMix m, uint64_t* h, bool inverse,
              hipStream_t st);
size_t scan_temp_bytes(int64_t n);
void inclusive_scan_i32(void* temp, size_t temp_bytes, const int32_t* in, int32_t* out,
                        int64_t n, hipStream_t st);
// sorted hs -> unique keys, segment starts, local columns; zero_a / zero_b (may be
// null): n floats each to clear in the same pass
void rle(const uint64_t* hs, const int32_t* pos_s, int64_t n, int32_t* flags, int32_t* segid,
         void* scan_temp, size_t scan_bytes, uint64_t* uniq, int32_t* seg_start,
         int32_t* local_col, int32_t* n_uniq, float* zero_a, float* zero_b, hipStream_t st);
// counts[u] = min(segment length, sat); cap: capacity of counts
void seg_counts(const int32_t* seg_start, const int32_t* n_uniq, int64_t cap, uint8_t* counts,
                int sat, hipStream_t st);
// bounds: [G + 1] key ranges; n_uniq may be null (then n_host keys); offsets: [G + 1]
void owner_split(const uint64_t* uniq, const int32_t* n_uniq, int64_t n_host,
                 const uint64_t* bounds, int G, int64_t* offsets, hipStream_t st);
void owner_of(const uint64_t* h, int64_t n, const uint64_t* bounds, int G, int32_t* owner,
              hipStream_t st);

}  // namespace psamd
