// Field-aware factorization machine (FFM, Juan et al. 2016): fused forward + backward on
// rows of a fixed width S <= 64, one wavefront per example.
//
//   m          = sum_i x_i w_i + sum_{i<j} x_i x_j <v_{i,f_j}, v_{j,f_i}>
//   G[i,f,:]   = sum_{j != i, f_j = f} x_j row_j[f_i k, + k)
//   m          = lin + 1/2 sum_i x_i <row_i, G[i]>          (the same G serves both)
//   dX0[i,f,:] = c x_i G[i,f,:],  c = -y sigma(-y m)
//
// The FM identity (pair sum = 1/2 (|sum v|^2 - sum |v|^2)) does not hold here: the vector a
// position contributes depends on its partner, so the pairs are visited, and the backward is
// a transpose-gather inside the row. All of it runs on one LDS tile per wave:
//
// * Stage: lane j < S loads row j (Dr / 8 16-B loads, four in flight) into the wave's tile
//   [S][Q] of 16-B chunks, Q = Dr / 8 made odd, so that the same chunk of neighbouring rows
//   lies in different bank groups; x_j beside it. No factor row is read from global twice.
// * Field lists: the host packs fields[] and its CSR (field -> positions) into bytes of the
//   kernel argument (49 words); the block copies them to LDS once. A gradient cell (i, f)
//   is then summed by exactly one lane, in list order: no LDS atomics, a fixed sum order.
// * One loop: a work item is (position i, 16-B chunk c) = 8 / k whole fields; items are
//   dealt round-robin, i fastest, so the lanes of a wave mostly share c and with it the
//   lists they walk. For each field f of the chunk the lane walks f's positions j != i, reads
//   k bf16 at tile[j][f_i k] (lanes with different f_i: different banks; the same f_i: one
//   broadcast address) and adds x_j times them into 8 fp32 G values. The item's share of
//   the margin is x_i <tile[i][c], G>.
// * G of a lane's first KEEP items stays in registers across the margin reduction and the
//   loss; later items are computed again from the tile (LDS reads only). dX0[i][c] leaves
//   as one 16-B store by the item's lane; chunks past F k store zeros.
// * Loss, accuracy, AUC bin, coef: once per row by lane 0, as fm_csr_kernel.
//
// The tile belongs to its wave: the only block barrier is the one after the field lists are
// copied, before the row loop. kBwd = false writes margins[B] and nothing else.
#include "ffm.h"
#include "bf16.cuh"
#include "common.cuh"

#include <algorithm>
#include <stdexcept>
#include <string>

namespace psamd {

namespace {

constexpr int kMapWords = 49;   // bytes: fld[64] | pos[64] | off[65 -> 68]
constexpr int kMapChunks = 16;  // the block's copy: 256 B of LDS in front of the tiles
constexpr int kXsChunks = 16;   // x of a wave's 64 positions behind its tile

struct FfmK {
  Ffm a;
  int C, Q, items;  // 16-B chunks of a row, the tile's row stride in chunks (odd), S * C
  uint32_t map[kMapWords];
};

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
struct alignas(K * 2) FfmVec {  // k bf16 of one field, as the tile holds them
  uint32_t w[K / 2];
};

// G of item t = (i, c) and its share x_i <tile[i][c], G> of the pair sum
template <int K>
__device__ __forceinline__ float ffm_item(const FfmK& p, const FfmLds& l, int t, float (&G)[8]) {
  const int c = t / p.a.S, i = t - c * p.a.S;
  const char* col = reinterpret_cast<const char*>(l.tile) + (int)l.fld[i] * (K * 2);
#pragma unroll
  for (int e = 0; e < 8; ++e) G[e] = 0.f;
#pragma unroll
  for (int u = 0; u < 8 / K; ++u) {
    const int f = c * (8 / K) + u;
    if (f < p.a.F) {
      const int q1 = l.off[f + 1];
      for (int q = l.off[f]; q < q1; ++q) {
        const int j = l.pos[q];
        if (j == i) continue;
        const float xj = l.xs[j];
        const FfmVec<K> v = *reinterpret_cast<const FfmVec<K>*>(col + j * p.Q * 16);
#pragma unroll
        for (int e = 0; e < K / 2; ++e) {
          G[u * K + 2 * e] = fmaf(xj, __uint_as_float(v.w[e] << 16), G[u * K + 2 * e]);
          G[u * K + 2 * e + 1] = fmaf(xj, __uint_as_float(v.w[e] & 0xffff0000u), G[u * K + 2 * e + 1]);
        }
      }
    }
  }
  const uint4 own = l.tile[i * p.Q + c];
  const uint32_t ow[4] = {own.x, own.y, own.z, own.w};
  float dot = 0.f;
#pragma unroll
  for (int e = 0; e < 4; ++e) {
    dot = fmaf(__uint_as_float(ow[e] << 16), G[2 * e], dot);
    dot = fmaf(__uint_as_float(ow[e] & 0xffff0000u), G[2 * e + 1], dot);
  }
  return l.xs[i] * dot;
}

// dX0[b * S + i][c] = bf16(coef x_i G): one 16-B store
__device__ __forceinline__ void ffm_store(const FfmK& p, const FfmLds& l, int64_t b, int t,
                                          float coef, const float (&G)[8]) {
  const int c = t / p.a.S, i = t - c * p.a.S;
  const float s = coef * l.xs[i];
  uint32_t o[4];
#pragma unroll
  for (int e = 0; e < 4; ++e)
    o[e] = (uint32_t)f32_to_bf16(s * G[2 * e]) | ((uint32_t)f32_to_bf16(s * G[2 * e + 1]) << 16);
  uint4* dst = reinterpret_cast<uint4*>((uint16_t*)p.a.dX0 + (b * p.a.S + i) * p.a.Dr);
  dst[c] = make_uint4(o[0], o[1], o[2], o[3]);
}

template <int K, int KEEP, bool kBwd>
__global__ void __launch_bounds__(256) ffm_kernel(const FfmK p) {
  extern __shared__ uint4 smem[];
  if (threadIdx.x == 0) {
    uint32_t* mw = reinterpret_cast<uint32_t*>(smem);
#pragma unroll
    for (int w = 0; w < kMapWords; ++w) mw[w] = p.map[w];
  }
  __syncthreads();
  const Ffm& a = p.a;
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6, W = blockDim.x >> 6;
  const int S = a.S;
  FfmLds l;
  l.fld = reinterpret_cast<const uint8_t*>(smem);
  l.pos = l.fld + 64;
  l.off = l.fld + 128;
  l.tile = smem + kMapChunks + wv * (S * p.Q + kXsChunks);
  l.xs = reinterpret_cast<float*>(l.tile + S * p.Q);
  double loss_acc = 0, corr_acc = 0, cnt = 0;
  for (int64_t b = blockIdx.x * (int64_t)W + wv; b < a.B; b += (int64_t)gridDim.x * W) {
    float lin = 0.f;
    if (lane < S) {
      const int64_t pp = b * S + lane;
      const float x = a.vals ? a.vals[pp] : 1.f;
      const int64_t col = a.local_col ? (int64_t)a.local_col[pp] : pp;
      const float w = in_range(col, a.w_cap) ? a.w_local[col] : 0.f;
      int64_t r = col;
      if (a.idx) r = in_range(r, a.idx_cap) ? a.idx[r] : -1;
      const bool ok = in_range(r, a.rows_cap);  // unresolved key: zero row
      const uint4* src = reinterpret_cast<const uint4*>((const uint16_t*)a.rows + (ok ? r : 0) * a.Dr);
      uint4* dst = l.tile + lane * p.Q;
      for (int c0 = 0; c0 < p.C; c0 += 4) {
        uint4 q[4];
#pragma unroll
        for (int u = 0; u < 4; ++u)
          q[u] = ok && c0 + u < p.C ? src[c0 + u] : make_uint4(0, 0, 0, 0);
#pragma unroll
        for (int u = 0; u < 4; ++u)
          if (c0 + u < p.C) dst[c0 + u] = q[u];
      }
      l.xs[lane] = x;
      lin = w * x;
    }
    wave_lds_sync();
    float Gk[KEEP > 0 ? KEEP : 1][8];
    float part = 0.f;
#pragma unroll
    for (int n = 0; n < KEEP; ++n) {
      const int t = lane + 64 * n;
      if (t < p.items) part += ffm_item<K>(p, l, t, Gk[n]);
    }
    for (int t = lane + 64 * KEEP; t < p.items; t += 64) {
      float G[8];
      part += ffm_item<K>(p, l, t, G);
    }
    const float m = wave_allsum(lin + 0.5f * part);
    if (!kBwd) {
      if (lane == 0) a.margins[b] = m;
      wave_lds_sync();  // the next row's stage writes the tile this one read
      continue;
    }
    const float y = a.labels[b] > 0.f ? 1.f : -1.f;
    const float ym = y * m;
    const float coef = -y / (1.f + expf(ym));
#pragma unroll
    for (int n = 0; n < KEEP; ++n) {
      const int t = lane + 64 * n;
      if (t < p.items) ffm_store(p, l, b, t, coef, Gk[n]);
    }
    for (int t = lane + 64 * KEEP; t < p.items; t += 64) {
      float G[8];
      ffm_item<K>(p, l, t, G);
      ffm_store(p, l, b, t, coef, G);
    }
    if (lane == 0) {
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
    wave_lds_sync();
  }
  if (kBwd && a.metrics) {  // per-wave DPP sums, lane 63 adds (no barriers)
    const double ls = wave_sum_dpp(loss_acc), c = wave_sum_dpp(corr_acc), n = wave_sum_dpp(cnt);
    if (lane == 63 && n > 0) {
      double* mt = acc_stripe(a.metrics, a.acc_stripes);
      atomicAdd(&mt[0], ls);
      atomicAdd(&mt[1], c);
      atomicAdd(&mt[2], n);
    }
  }
}

// G of a lane's first kKeep items stays in registers between the passes. The compiler
// overlaps the unrolled items, so a kept item costs ~23 VGPRs, not 8: the training form
// takes 87 VGPRs at 2 (5 waves / SIMD, which is also what the LDS of a Criteo tile at k = 2
// allows), 133 at 4 (3 waves), 151 at 6, 187 at 8 (2 waves). 2 it is, chosen by occupancy;
// the alternatives have not been timed.
constexpr int kKeep = 2;

template <bool kBwd>
void ffm_launch(const Ffm& a, hipStream_t st) {
  auto bad = [](const std::string& s) { throw std::invalid_argument("ffm: " + s); };
  if (a.S < 1 || a.S > 64) bad("1..64 positions per row, not " + std::to_string(a.S));
  if (a.k != 2 && a.k != 4 && a.k != 8) bad("k in {2, 4, 8}, not " + std::to_string(a.k));
  if (a.Dr % 8 || a.Dr > 128 || a.F < 1 || a.F * a.k > a.Dr)
    bad("rows of F * k <= Dr <= 128 columns, Dr % 8 == 0 (F = " + std::to_string(a.F) +
        ", k = " + std::to_string(a.k) + ", Dr = " + std::to_string(a.Dr) + ")");
  if (!a.fields) bad("no field map");
  for (int i = 0; i < a.S; ++i)
    if (a.fields[i] < 0 || a.fields[i] >= a.F)
      bad("field " + std::to_string(a.fields[i]) + " of position " + std::to_string(i) +
          " outside [0, " + std::to_string(a.F) + ")");
  if (a.B <= 0) return;
  FfmK p = {};
  p.a = a;
  p.a.fields = nullptr;
  p.C = a.Dr / 8;
  p.Q = p.C | 1;
  p.items = a.S * p.C;
  uint8_t* mb = reinterpret_cast<uint8_t*>(p.map);  // fld | pos | off, positions in row order
  int n = 0;
  for (int f = 0; f < a.F && f < 64; ++f) {
    mb[128 + f] = (uint8_t)n;
    for (int i = 0; i < a.S; ++i)
      if (a.fields[i] == f) mb[64 + n++] = (uint8_t)i;
  }
  for (int f = std::min(a.F, 64); f <= 64; ++f) mb[128 + f] = (uint8_t)n;
  for (int i = 0; i < a.S; ++i) mb[i] = (uint8_t)a.fields[i];
  // as many waves (rows) per block as 64 KB of LDS hold, four at the most
  const int wave_bytes = (a.S * p.Q + kXsChunks) * 16;
  const int W = std::min(4, (65536 - kMapChunks * 16) / wave_bytes);
  const size_t lds = kMapChunks * 16 + (size_t)W * wave_bytes;
  const unsigned g = (unsigned)std::min<int64_t>((a.B + 2 * W - 1) / (2 * W), 1 << 16);
#define PSAMD_FFM(KK) \
  if (a.k == KK) ffm_kernel<KK, kBwd ? kKeep : 0, kBwd><<<g, 64 * W, lds, st>>>(p)
  PSAMD_FFM(2);
  PSAMD_FFM(4);
  PSAMD_FFM(8);
#undef PSAMD_FFM
  PSAMD_HIP_CHECK(hipGetLastError());
}

}  // namespace

void ffm_fwd_bwd(const Ffm& a, hipStream_t st) { ffm_launch<true>(a, st); }
void ffm_margins(const Ffm& a, hipStream_t st) { ffm_launch<false>(a, st); }

}  // namespace psamd
