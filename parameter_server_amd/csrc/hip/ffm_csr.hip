// FFM on CSR rows with a field per occurrence (libffm's field:index:value rows, what the
// device text parsers emit): rows of any width, fields missing, repeated and in any order.
// The maths is ffm.hip's with f_i = fld[p_i]; an occurrence whose field is outside [0, F)
// keeps its linear term and takes part in no pair (its dX0 row is zero).
//
// Two launches, so that the tile kernel keeps the fixed-width kernel's registers:
//
// ffm_csr_kernel: one wavefront per row of n <= T positions, on a per-wave LDS region
//   [fld | pos | off bytes, 256 B][tile T x Q chunks][x, 256 B], grid-stride over B.
//   * Stage: lane j < n loads row j into the tile (ffm_stage, as ffm.hip) and writes
//     row_of[p] = b.
//   * Field lists, rebuilt for every row inside the wave, no LDS atomics: a stable counting
//     sort of the n positions by field. The wave loops over the row's DISTINCT fields: the
//     field fs of the lowest unserved lane (readlane), a ballot of the lanes that hold it;
//     such a lane's rank is popcount(ballot & lanes below), and lane fs keeps the field's
//     count in a register. One inclusive shuffle scan over the 64 lanes (= fields) gives
//     off[], a lane fetches off[f] from lane f by one more shuffle and writes its position
//     at pos[off[f] + rank]. All of it is registers and cross-lane moves; the only LDS
//     traffic is the final byte stores, and one wave sync (the tile's) covers them.
//     Lists are in position order, so a gradient cell (i, f) is summed by one lane in
//     ascending j: the fixed-width kernel's fixed sum order.
//   * An occurrence with a field outside [0, F) is in no list and enters the tile with
//     x = 0 and field 0 (its linear term w x is kept in a register): every product it
//     takes part in is then 0, with no branch in the item loop.
//   * The item loop is ffm_item / ffm_store of ffm_tile.cuh with the row's n in place of S:
//     items (i, c), t = lane + 64 m, i fastest; G of the first kKeep items stays in
//     registers across the margin reduction.
//   Rows wider than T are left alone by this kernel.
//
// ffm_csr_wide_kernel: the rows with n > T, any width, partners read from global memory.
//   A wave takes 64 rows' widths at a time (one row_ptr pair per lane), ballots the wide
//   ones and serves them one after the other with all its lanes: a minibatch without wide
//   rows costs B / 64 wave iterations. The same item-to-lane dealing; item (i, c) walks all
//   j != i of the row in ascending j, keeps those with fld[j] in the chunk's fields and reads
//   the k bf16 at row_j[f_i k] through the local_col / idx chain. Ascending j filtered by
//   field IS the list order, the fmaf sequence per cell is the same, and so are the
//   reductions: a row of n <= 64 gives the same bits on either path.
//
// Loss, accuracy, AUC bin, coef: once per row by lane 0 (an empty row has m = 0 and is
// counted). kBwd = false writes margins[B] and nothing else.
#include "ffm.h"
#include "ffm_tile.cuh"

#include <algorithm>
#include <stdexcept>
#include <string>

namespace psamd {

namespace {

struct FfmCsrK {
  FfmCsr a;
  int C, Q;  // 16-B chunks of a row, the tile's row stride in chunks (odd)
};

// row b's positions [lo, lo + n), both ends clamped to nnz (as fm_csr_kernel)
__device__ __forceinline__ int ffm_csr_row(const FfmCsr& a, int64_t b, int64_t& lo) {
  lo = a.row_ptr[b];
  int64_t hi = a.row_ptr[b + 1];
  lo = lo < 0 ? 0 : (lo > a.nnz ? a.nnz : lo);
  hi = hi < lo ? lo : (hi > a.nnz ? a.nnz : hi);
  return (int)(hi - lo);  // nnz < 2^31
}

template <int K, int KEEP, bool kBwd>
__global__ void __launch_bounds__(256) ffm_csr_kernel(const FfmCsrK p) {
  extern __shared__ uint4 smem[];
  const FfmCsr& a = p.a;
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6, W = blockDim.x >> 6;
  uint4* region = smem + wv * (kFfmMapChunks + a.T * p.Q + kFfmXsChunks);
  uint8_t* map = reinterpret_cast<uint8_t*>(region);
  FfmLds l;
  l.fld = map;
  l.pos = map + 64;
  l.off = map + 128;
  l.tile = region + kFfmMapChunks;
  l.xs = reinterpret_cast<float*>(l.tile + a.T * p.Q);
  const uint64_t below = (1ull << lane) - 1;
  double loss_acc = 0, corr_acc = 0, cnt = 0;
  for (int64_t b = blockIdx.x * (int64_t)W + wv; b < a.B; b += (int64_t)gridDim.x * W) {
    int64_t lo;
    const int n = ffm_csr_row(a, b, lo);
    if (n > a.T) continue;  // ffm_csr_wide_kernel's
    float lin = 0.f;
    int f = -1;
    if (lane < n) {
      float x, w;
      bool ok;
      const uint4* src = ffm_src(a, lo + lane, x, w, ok);
      ffm_stage(src, ok, l.tile + lane * p.Q, p.C);
      lin = w * x;
      f = a.fld[lo + lane];
      if (!in_range(f, a.F)) f = -1, x = 0.f;
      l.xs[lane] = x;
      map[lane] = (uint8_t)(f < 0 ? 0 : f);
      if (kBwd) a.row_of[lo + lane] = (int32_t)b;
    }
    // counting sort by field: rank among earlier lanes of the same field, counts by field
    int rank = 0, mine = 0;
    for (uint64_t todo = __ballot(f >= 0); todo;) {
      const int fs = __builtin_amdgcn_readlane(f, __ffsll((unsigned long long)todo) - 1);
      const uint64_t same = __ballot(f == fs);
      if (f == fs) rank = __popcll(same & below);
      if (lane == fs) mine = __popcll(same);
      todo &= ~same;
    }
    int incl = mine;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
      const int up = __shfl_up(incl, d, 64);
      if (lane >= d) incl += up;
    }
    const int base = __shfl(incl - mine, f < 0 ? 0 : f, 64);  // off[f]
    map[128 + 1 + lane] = (uint8_t)incl;
    if (lane == 0) map[128] = 0;
    if (f >= 0) map[64 + base + rank] = (uint8_t)lane;
    wave_lds_sync();
    const int items = n * p.C;
    float Gk[KEEP > 0 ? KEEP : 1][8];
    float part = 0.f;
#pragma unroll
    for (int k = 0; k < KEEP; ++k) {
      const int t = lane + 64 * k;
      if (t < items) part += ffm_item<K>(l, n, p.Q, a.F, t, Gk[k]);
    }
    for (int t = lane + 64 * KEEP; t < items; t += 64) {
      float G[8];
      part += ffm_item<K>(l, n, p.Q, a.F, t, G);
    }
    const float m = wave_allsum(lin + 0.5f * part);
    if (!kBwd) {
      if (lane == 0) a.margins[b] = m;
      wave_lds_sync();  // the next row's stage writes the tile this one read
      continue;
    }
    const float y = a.labels[b] > 0.f ? 1.f : -1.f;
    const float coef = -y / (1.f + expf(y * m));
#pragma unroll
    for (int k = 0; k < KEEP; ++k) {
      const int t = lane + 64 * k;
      if (t < items) {
        const int c = t / n, i = t - c * n;
        ffm_store(a.dX0, lo + i, a.Dr, c, coef * l.xs[i], Gk[k]);
      }
    }
    for (int t = lane + 64 * KEEP; t < items; t += 64) {
      float G[8];
      ffm_item<K>(l, n, p.Q, a.F, t, G);
      const int c = t / n, i = t - c * n;
      ffm_store(a.dX0, lo + i, a.Dr, c, coef * l.xs[i], G);
    }
    if (lane == 0) ffm_row_done(a, b, y, m, coef, loss_acc, corr_acc, cnt);
    wave_lds_sync();
  }
  if (kBwd && a.metrics) ffm_metrics(a, loss_acc, corr_acc, cnt);
}

// G of item t = (i, c) of the row [lo, lo + n) from global memory, its share of the pair
// sum, and x_i (0 for a field outside [0, F), as the tile holds it)
template <int K>
__device__ __forceinline__ float ffm_wide_item(const FfmCsr& a, int64_t lo, int n, int64_t t,
                                               float (&G)[8], float& xi) {
  const int c = (int)(t / n), i = (int)(t - (int64_t)c * n);
  float wi;
  bool oki;
  const uint4* own = ffm_src(a, lo + i, xi, wi, oki);
  int fi = a.fld[lo + i];
  if (!in_range(fi, a.F)) fi = 0, xi = 0.f;
  const int f0 = c * (8 / K);
#pragma unroll
  for (int e = 0; e < 8; ++e) G[e] = 0.f;
  for (int j = 0; j < n; ++j) {
    const int fj = a.fld[lo + j];
    if (j == i || fj < f0 || fj >= f0 + 8 / K || fj >= a.F) continue;
    float xj, wj;
    bool ok;
    const uint4* src = ffm_src(a, lo + j, xj, wj, ok);
    FfmVec<K> v = {};
    if (ok) v = *reinterpret_cast<const FfmVec<K>*>(reinterpret_cast<const char*>(src) + fi * (K * 2));
#pragma unroll
    for (int u = 0; u < 8 / K; ++u)
      if (fj == f0 + u) ffm_fma<K>(xj, v, u, G);
  }
  return xi * ffm_dot(oki ? own[c] : make_uint4(0, 0, 0, 0), G);
}

template <int K, bool kBwd>
__global__ void __launch_bounds__(256) ffm_csr_wide_kernel(const FfmCsrK p) {
  const FfmCsr& a = p.a;
  const int lane = threadIdx.x & 63;
  const int64_t wave = blockIdx.x * (int64_t)(blockDim.x >> 6) + (threadIdx.x >> 6);
  const int64_t waves = (int64_t)gridDim.x * (blockDim.x >> 6);
  double loss_acc = 0, corr_acc = 0, cnt = 0;
  for (int64_t b0 = wave * 64; b0 < a.B; b0 += waves * 64) {
    int64_t lo_l = 0;
    const int n_l = b0 + lane < a.B ? ffm_csr_row(a, b0 + lane, lo_l) : 0;
    for (uint64_t wide = __ballot(n_l > a.T); wide; wide &= wide - 1) {
      const int s = __ffsll((unsigned long long)wide) - 1;
      const int64_t b = b0 + s;
      const int n = __builtin_amdgcn_readlane(n_l, s);
      const int64_t lo = ((int64_t)__builtin_amdgcn_readlane((int)(lo_l >> 32), s) << 32) |
                         (uint32_t)__builtin_amdgcn_readlane((int)lo_l, s);
      float lin = 0.f;
      for (int j = lane; j < n; j += 64) {
        const float x = a.vals ? a.vals[lo + j] : 1.f;
        const int64_t col = a.local_col ? (int64_t)a.local_col[lo + j] : lo + j;
        lin += (in_range(col, a.w_cap) ? a.w_local[col] : 0.f) * x;
        if (kBwd) a.row_of[lo + j] = (int32_t)b;
      }
      const int64_t items = (int64_t)n * p.C;
      float part = 0.f;
      for (int64_t t = lane; t < items; t += 64) {
        float G[8], xi;
        part += ffm_wide_item<K>(a, lo, n, t, G, xi);
      }
      const float m = wave_allsum(lin + 0.5f * part);
      if (!kBwd) {
        if (lane == 0) a.margins[b] = m;
        continue;
      }
      const float y = a.labels[b] > 0.f ? 1.f : -1.f;
      const float coef = -y / (1.f + expf(y * m));
      for (int64_t t = lane; t < items; t += 64) {
        float G[8], xi;
        ffm_wide_item<K>(a, lo, n, t, G, xi);
        const int c = (int)(t / n);
        ffm_store(a.dX0, lo + (t - (int64_t)c * n), a.Dr, c, coef * xi, G);
      }
      if (lane == 0) ffm_row_done(a, b, y, m, coef, loss_acc, corr_acc, cnt);
    }
  }
  if (kBwd && a.metrics) ffm_metrics(a, loss_acc, corr_acc, cnt);
}

constexpr int kKeep = 2;  // as ffm.hip: the third kept item would cost the fifth wave / SIMD

template <bool kBwd>
void ffm_csr_launch(const FfmCsr& a, hipStream_t st) {
  auto bad = [](const std::string& s) { throw std::invalid_argument("ffm_csr: " + s); };
  if (a.T < 1 || a.T > 64) bad("tile of 1..64 rows, not " + std::to_string(a.T));
  if (a.k != 2 && a.k != 4 && a.k != 8) bad("k in {2, 4, 8}, not " + std::to_string(a.k));
  if (a.Dr % 8 || a.Dr > 128 || a.F < 1 || a.F * a.k > a.Dr)
    bad("rows of F * k <= Dr <= 128 columns, Dr % 8 == 0 (F = " + std::to_string(a.F) +
        ", k = " + std::to_string(a.k) + ", Dr = " + std::to_string(a.Dr) + ")");
  if (a.nnz < 0 || a.nnz >= (int64_t(1) << 31)) bad("0 <= nnz < 2^31");
  if (!a.row_ptr || (a.nnz > 0 && !a.fld)) bad("no row_ptr / fld");
  if (a.B <= 0) return;
  FfmCsrK p = {};
  p.a = a;
  p.C = a.Dr / 8;
  p.Q = p.C | 1;
  // as many waves (rows) per block as 64 KB of LDS hold, four at the most
  const int wave_bytes = (kFfmMapChunks + a.T * p.Q + kFfmXsChunks) * 16;
  const int W = std::min(4, 65536 / wave_bytes);
  const unsigned g = (unsigned)std::min<int64_t>((a.B + 2 * W - 1) / (2 * W), 1 << 16);
  // the wide rows: 64 rows' widths per wave iteration
  const unsigned gw = (unsigned)std::min<int64_t>((a.B + 255) / 256, 1 << 16);
#define PSAMD_FFM_CSR(KK)                                                                   \
  if (a.k == KK) {                                                                          \
    ffm_csr_kernel<KK, kBwd ? kKeep : 0, kBwd><<<g, 64 * W, (size_t)W * wave_bytes, st>>>(p); \
    ffm_csr_wide_kernel<KK, kBwd><<<gw, 256, 0, st>>>(p);                                   \
  }
  PSAMD_FFM_CSR(2);
  PSAMD_FFM_CSR(4);
  PSAMD_FFM_CSR(8);
#undef PSAMD_FFM_CSR
  PSAMD_HIP_CHECK(hipGetLastError());
}

}  // namespace

void ffm_csr(const FfmCsr& a, hipStream_t st) { ffm_csr_launch<true>(a, st); }
void ffm_csr_margins(const FfmCsr& a, hipStream_t st) { ffm_csr_launch<false>(a, st); }

}  // namespace psamd
