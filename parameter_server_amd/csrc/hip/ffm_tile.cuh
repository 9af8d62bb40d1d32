// What the FFM tile kernels share (ffm.hip: rows of a fixed width with one field map;
// ffm_csr.hip: CSR rows with a field per occurrence): a wave's view of its LDS, the staging of
// one factor row into the tile, the item loop's body and store, and the per-row loss.
#pragma once
#include "bf16.cuh"
#include "common.cuh"

namespace psamd {

constexpr int kFfmMapChunks = 16;  // bytes fld[64] | pos[64] | off[65 -> 68], padded to 256 B
constexpr int kFfmXsChunks = 16;   // x of a wave's 64 positions behind its tile

struct FfmLds {  // a wave's view of the block's LDS
  const uint8_t *fld, *pos, *off;
  uint4* tile;
  float* xs;
};

// LDS written by some lanes of the wave is read by others of the same wave
__device__ __forceinline__ void wave_lds_sync() {
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
}

template <int K>
struct alignas(K * 2) FfmVec {  // k bf16 of one field, as a row holds them
  uint32_t w[K / 2];
};

// Occurrence pp of argument struct A (Ffm / FfmCsr): its value, its wide weight and its
// factor row (ok false: an unresolved key or a column out of range, which is a zero row;
// the pointer is then row 0's and must not be read).
template <class A>
__device__ __forceinline__ const uint4* ffm_src(const A& a, int64_t pp, float& x, float& w,
                                                bool& ok) {
  x = a.vals ? a.vals[pp] : 1.f;
  const int64_t col = a.local_col ? (int64_t)a.local_col[pp] : pp;
  w = in_range(col, a.w_cap) ? a.w_local[col] : 0.f;
  int64_t r = col;
  if (a.idx) r = in_range(r, a.idx_cap) ? a.idx[r] : -1;
  ok = in_range(r, a.rows_cap);
  return reinterpret_cast<const uint4*>((const uint16_t*)a.rows + (ok ? r : 0) * a.Dr);
}

// C 16-B chunks of a factor row into the tile, four loads in flight (!ok: zeros)
__device__ __forceinline__ void ffm_stage(const uint4* src, bool ok, uint4* dst, int C) {
  for (int c0 = 0; c0 < C; c0 += 4) {
    uint4 q[4];
#pragma unroll
    for (int u = 0; u < 4; ++u) q[u] = ok && c0 + u < C ? src[c0 + u] : make_uint4(0, 0, 0, 0);
#pragma unroll
    for (int u = 0; u < 4; ++u)
      if (c0 + u < C) dst[c0 + u] = q[u];
  }
}

// G[u k + e] += x_j v[e] for the k bf16 of one partner
template <int K>
__device__ __forceinline__ void ffm_fma(float xj, const FfmVec<K>& v, int u, float (&G)[8]) {
#pragma unroll
  for (int e = 0; e < K / 2; ++e) {
    G[u * K + 2 * e] = fmaf(xj, __uint_as_float(v.w[e] << 16), G[u * K + 2 * e]);
    G[u * K + 2 * e + 1] = fmaf(xj, __uint_as_float(v.w[e] & 0xffff0000u), G[u * K + 2 * e + 1]);
  }
}

// <own chunk, G>: the item's share of the pair sum, before x_i
__device__ __forceinline__ float ffm_dot(const uint4 own, const float (&G)[8]) {
  const uint32_t ow[4] = {own.x, own.y, own.z, own.w};
  float dot = 0.f;
#pragma unroll
  for (int e = 0; e < 4; ++e) {
    dot = fmaf(__uint_as_float(ow[e] << 16), G[2 * e], dot);
    dot = fmaf(__uint_as_float(ow[e] & 0xffff0000u), G[2 * e + 1], dot);
  }
  return dot;
}

// G of item t = (i, c) of a row of n positions (tile rows of Q chunks, F fields) and its
// share x_i <tile[i][c], G> of the pair sum
template <int K>
__device__ __forceinline__ float ffm_item(const FfmLds& l, int n, int Q, int F, int t,
                                          float (&G)[8]) {
  const int c = t / n, i = t - c * n;
  const char* col = reinterpret_cast<const char*>(l.tile) + (int)l.fld[i] * (K * 2);
#pragma unroll
  for (int e = 0; e < 8; ++e) G[e] = 0.f;
#pragma unroll
  for (int u = 0; u < 8 / K; ++u) {
    const int f = c * (8 / K) + u;
    if (f < F) {
      const int q1 = l.off[f + 1];
      for (int q = l.off[f]; q < q1; ++q) {
        const int j = l.pos[q];
        if (j == i) continue;
        ffm_fma<K>(l.xs[j], *reinterpret_cast<const FfmVec<K>*>(col + j * Q * 16), u, G);
      }
    }
  }
  return l.xs[i] * ffm_dot(l.tile[i * Q + c], G);
}

// dX0[row][c] = bf16(s G), s = coef x_i: one 16-B store
__device__ __forceinline__ void ffm_store(void* dX0, int64_t row, int Dr, int c, float s,
                                          const float (&G)[8]) {
  uint32_t o[4];
#pragma unroll
  for (int e = 0; e < 4; ++e)
    o[e] = (uint32_t)f32_to_bf16(s * G[2 * e]) | ((uint32_t)f32_to_bf16(s * G[2 * e + 1]) << 16);
  uint4* dst = reinterpret_cast<uint4*>((uint16_t*)dX0 + row * Dr);
  dst[c] = make_uint4(o[0], o[1], o[2], o[3]);
}

// One row's coef, loss, accuracy and AUC bin (called by one lane)
template <class A>
__device__ __forceinline__ void ffm_row_done(const A& a, int64_t b, float y, float m, float coef,
                                             double& loss_acc, double& corr_acc, double& cnt) {
  const float ym = y * m;
  a.coef[b] = coef;
  loss_acc += ym > 20.f ? expf(-ym) : (ym < -20.f ? -ym : log1pf(expf(-ym)));
  corr_acc += ((y > 0.f) == (m > 0.f)) ? 1.0 : 0.0;
  cnt += 1.0;
  if (a.hist) {
    const float pr = 1.f / (1.f + expf(-m));
    const float pb = pr == pr ? fminf(fmaxf(pr * a.nbins, 0.f), (float)(a.nbins - 1)) : 0.f;
    atomicAdd(&a.hist[(y > 0.f ? a.nbins : 0) + (int)pb], 1u);
  }
}

// per-wave DPP sums, lane 63 adds (no barriers)
template <class A>
__device__ __forceinline__ void ffm_metrics(const A& a, double loss_acc, double corr_acc,
                                            double cnt) {
  const double ls = wave_sum_dpp(loss_acc), c = wave_sum_dpp(corr_acc), n = wave_sum_dpp(cnt);
  if ((threadIdx.x & 63) == 63 && n > 0) {
    double* mt = acc_stripe(a.metrics, a.acc_stripes);
    atomicAdd(&mt[0], ls);
    atomicAdd(&mt[1], c);
    atomicAdd(&mt[2], n);
  }
}

}  // namespace psamd
