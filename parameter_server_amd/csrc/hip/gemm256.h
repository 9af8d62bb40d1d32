// Host entry points of gemm256.hip: the 256 x 256 LDS-DMA bf16 GEMMs. Operands 16-B
// aligned, K a multiple of 64.
#pragma once
#include <hip/hip_runtime.h>
#include <cstdint>

namespace psamd {

// out [M, N] f32 = beta out + A^T B for MN-major A [K, M], B [K, N]: split-K partials
// into part [splits, M, N], then a fixed-order sum. phase 0 both / 1 GEMM / 2 reduce /
// 3 reduce in the GEMM (tile_ctr: one zeroed word per tile, else may be null)
void gemm_tn256(const __bf16* A, int64_t lda, const __bf16* B, int64_t ldb, int M, int N, int K,
                int splits, float* part, float* out, float beta, int phase, unsigned int* tile_ctr,
                hipStream_t st);
// R, C multiples of 64
void transpose_bf16(const void* in, int R, int C, void* out, hipStream_t st);
// K-major A [M, K], B [N, K]; bias may be null; C (bf16) / Cf (f32): one non-null
void gemm_nt256(const __bf16* A, int64_t lda, const __bf16* B, int64_t ldb, int M, int N, int K,
                const float* bias, bool relu, __bf16* C, int64_t ldc, float* Cf, int64_t ldcf,
                int variant, hipStream_t st);

}  // namespace psamd
