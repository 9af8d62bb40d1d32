// Host entry points of bcd.hip: Darlin block coordinate descent. CSC of one rank: col /
// row int32 per nnz (sorted by col), val f32 per nnz or null (binary). A block is the nnz
// range [p0, p1) holding global columns [c0, c0 + ncols); nrows examples.
#pragma once
#include <hip/hip_runtime.h>
#include <cstdint>

namespace psamd {

void bcd_grad(const int32_t* col, const int32_t* row, const float* val, int64_t p0, int64_t p1,
              int64_t c0, int64_t ncols, const double* ym, const float* y, int64_t nrows,
              const double* delta, const uint8_t* active, double* G, double* U, hipStream_t st);
// chunks: [nchunks + 1] entry offsets (bit 62 = hot chunk); rowq (2 doubles per
// example), urows (the block's distinct examples, needs rowq) may be null
void bcd_grad_chunked(const int32_t* col, const int32_t* row, const float* val,
                      const int64_t* chunks, int64_t nchunks, int64_t c0, int64_t ncols,
                      const double* ym, const float* y, int64_t nrows, const double* delta,
                      const uint8_t* active, double* rowq, double* G, double* U, bool zeroed,
                      bool rowq_ready, const int32_t* urows, int64_t nurows, hipStream_t st);
int bcd_rows_max_cols();  // LDS columns of the row kernels
int bcd_part_segments();
// dw non-null: the fused update (needs w, vio_bits, counter); k2: fixed-point shift
void bcd_grad_rows(const int32_t* col, const int32_t* row, const float* val, int64_t p0,
                   int64_t p1, int64_t c0, int64_t ncols, const double* ym, const float* y,
                   int64_t nrows, double* delta, uint8_t* active, int k2, int W,
                   long long* part, double* G, double* U, double* w, double* dw,
                   unsigned long long* vio_bits, unsigned int* counter, double eta, double lambda,
                   double delta_max, double kkt_thr, hipStream_t st);
// part2 (may be null): a narrow row pass's fixed-point sums, shift k2
void bcd_update(int64_t c0, int64_t ncols, double* G, double* U, double* w, double* delta,
                uint8_t* active, double* dw, double eta, double lambda, double delta_max,
                double kkt_thr, unsigned long long* vio_bits, bool consume, bool nan_filtered,
                const long long* part2, int k2, hipStream_t st);
void bcd_replica(int64_t c0, int64_t ncols, int64_t own0, int64_t own1, double* dw, double* w,
                 double* delta, uint8_t* active, double delta_max, hipStream_t st);
void bcd_dual(const int32_t* col, const int32_t* row, const float* val, int64_t p0, int64_t p1,
              int64_t c0, int64_t ncols, const double* dw, const float* y, double* ym,
              int64_t nrows, bool unique_rows, hipStream_t st);
// Row pass over dense per-row block layouts: the pending dual update of block j (jcol:
// column relative to the block, -1 none) fused with block k's gradient (narrow: part / G
// / U; wide: rowq). Every pointer from jcol on may be null.
void bcd_rowpass(int64_t n, double* ym, const float* y, const int32_t* jcol, const float* jval,
                 const double* jdw, int64_t jncols, const int32_t* kcol, const float* kval,
                 int64_t c0, int64_t ncols, const double* delta, const uint8_t* active, int k2,
                 int W, long long* part, double* G, double* U, double* rowq,
                 const int32_t* hcols, int64_t nhot, long long* part2_out, bool tau32,
                 hipStream_t st);
void bcd_objective(const double* ym, int64_t n, double* out, hipStream_t st);
// out: 3 doubles over columns [c0, c1)
void bcd_server_stats(const double* w, const uint8_t* active, int64_t c0, int64_t c1, double* out,
                      hipStream_t st);

}  // namespace psamd
