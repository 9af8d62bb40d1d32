// Host entry point of gemm.hip: C[m, n] = sum_k A(m, k) B(n, k) in bf16 with epilogues.
#pragma once
#include <hip/hip_runtime.h>

namespace psamd {

// A(m, k) = A[m * lda + k] if a_kmajor else A[k * lda + m] (B alike). epi bits: 1 bias,
// 4 mask by aux, 8 column sums. C (bf16) / Cf (f32): at least one non-null; splitk > 1:
// Cf only.
void gemm_bf16(bool a_kmajor, bool b_kmajor, const void* A, int lda, const void* B, int ldb,
               int M, int N, int K, int epi, const float* bias, const void* aux, int ldaux,
               void* C, int ldc, float* Cf, int ldcf, float beta, int splitk, float* colsum,
               hipStream_t st);

}  // namespace psamd
