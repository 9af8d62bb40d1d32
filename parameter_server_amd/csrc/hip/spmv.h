// Host entry point of spmv.hip: y = alpha * A x + beta * y over the compressed major
// dimension, gather (row-reduce) or scatter (atomic).
#pragma once
#include <hip/hip_runtime.h>
#include <cstdint>

namespace psamd {

// idx_bytes 4 / 8, val_bytes 4 / 8 (x, y and val alike); val may be null (binary)
void spmv(bool scatter, const int64_t* off, const void* idx, int idx_bytes, const void* val,
          int val_bytes, int64_t n_major, int64_t nnz, const void* x, int64_t n_x, double alpha,
          double beta, void* y, int64_t n_y, hipStream_t st);

}  // namespace psamd
