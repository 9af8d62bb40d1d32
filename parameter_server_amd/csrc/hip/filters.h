// Host entry points of filters.hip: CountMin over byte cells packed in u32 words (one
// region of rsize cells, or regions selected by key >> rshift; countmin.cuh), stream
// compaction, FixingFloat codes and the key-set signature. n_dev (may be null) is a
// device count that clamps n.
#pragma once
#include <hip/hip_runtime.h>
#include <cstdint>

namespace psamd {

// counts (may be null): per-key increments, else 1
void cm_insert(uint32_t* table, uint64_t rsize, int rshift, int k, uint32_t vmax,
               const uint64_t* keys, const uint8_t* counts, int64_t n, const int32_t* n_dev,
               hipStream_t st);
// keep[i] = count > freq; keep / out_count may be null
void cm_query(const uint32_t* table, uint64_t rsize, int rshift, int k, uint32_t vmax,
              const uint64_t* keys, int64_t n, const int32_t* n_dev, int freq, int32_t* keep,
              uint8_t* out_count, hipStream_t st);
// insert every unique key with its segment length
void cm_insert_seg(uint32_t* table, uint64_t rsize, int rshift, int k, uint32_t vmax,
                   const uint64_t* keys, const int32_t* seg_start, int64_t n, const int32_t* n_dev,
                   hipStream_t st);
// incl: inclusive scan of keep; remap may be null; keys_in / keys_out go together
void compact_kept(const int32_t* keep, const int32_t* incl, int64_t n, const int32_t* n_dev,
                  int32_t* kept_idx, int32_t* n_kept, int32_t* remap, const uint64_t* keys_in,
                  uint64_t* keys_out, hipStream_t st);
// mm: [min, max]
void ff_minmax(const float* x, int64_t n, float* mm, hipStream_t st);
// nbytes 1..7 per value
void ff_encode(const float* x, int64_t n, const float* mm, int nbytes, uint64_t seed,
               uint8_t* out, hipStream_t st);
void ff_decode(const uint8_t* code, int64_t n, const float* mm, int nbytes, float* out,
               hipStream_t st);
void key_signature(const uint64_t* keys, int64_t n, unsigned long long* sig, hipStream_t st);

}  // namespace psamd
