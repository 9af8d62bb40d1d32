// Host entry points of kvapi.hip: the k-value push / pull API. Rows [hdr 4 | keys C * kw
// | values C * k f32] of H words (pull rows: no values); G peers, off: [G + 1] offsets.
#pragma once
#include <hip/hip_runtime.h>
#include <cstdint>

namespace psamd {

// u_cap: capacity of seg_start - 1; kw 0 = key-less row of a registered key set
void kvv_pack_vals(const float* vals, int k, const int32_t* pos_s, const int32_t* seg_start,
                   const int32_t* n_uniq, int64_t u_cap, int64_t nnz, const int64_t* off, int G,
                   int64_t C, int kw, int64_t H, int32_t* send, hipStream_t st);
// table_vals: cap rows of k floats, `stride` floats apart
void kvv_serve(const int32_t* recv, int G, int64_t H, int64_t C, const int64_t* slot,
               const float* table_vals, int64_t cap, int k, int64_t stride, float* rec,
               hipStream_t st);
// op: 0 = add, 1 = assign
void kvv_apply(const int32_t* recv, int G, int64_t H, int64_t C, int kw, const int64_t* slot,
               float* table_vals, int64_t cap, int k, int op, hipStream_t st);
void kvv_unpack(const float* rec, int64_t C, int k, const int64_t* off, int G,
                const int32_t* local_col, int64_t nnz, float* out, hipStream_t st);
// off[0..1] = {0, *n_uniq}: the offsets of a single owner
void kvv_single_off(const int32_t* n_uniq, int64_t* off, hipStream_t st);

}  // namespace psamd
