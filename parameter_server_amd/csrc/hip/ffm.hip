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
// copied, before the row loop. kBwd = false writes margins[B] and nothing else. The staging,
// the item loop's body, the store and the per-row loss live in ffm_tile.cuh, shared with the
// CSR form (ffm_csr.hip: a field per occurrence, lists built per row in the wave).
#include "ffm.h"
#include "ffm_tile.cuh"

#include <algorithm>
#include <stdexcept>
#include <string>

namespace psamd {

namespace {

constexpr int kMapWords = 49;   // bytes: fld[64] | pos[64] | off[65 -> 68]
constexpr int kMapChunks = kFfmMapChunks;  // the block's copy: 256 B of LDS in front of the tiles
constexpr int kXsChunks = kFfmXsChunks;

struct FfmK {
  Ffm a;
  int C, Q, items;  // 16-B chunks of a row, the tile's row stride in chunks (odd), S * C
  uint32_t map[kMapWords];
};

// dX0[b * S + i][c] of item t = (i, c)
__device__ __forceinline__ void ffm_store_item(const FfmK& p, const FfmLds& l, int64_t b, int t,
                                               float coef, const float (&G)[8]) {
  const int c = t / p.a.S, i = t - c * p.a.S;
  ffm_store(p.a.dX0, b * p.a.S + i, p.a.Dr, c, coef * l.xs[i], G);
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
      float x, w;
      bool ok;
      const uint4* src = ffm_src(a, b * S + lane, x, w, ok);
      ffm_stage(src, ok, l.tile + lane * p.Q, p.C);
      l.xs[lane] = x;
      lin = w * x;
    }
    wave_lds_sync();
    float Gk[KEEP > 0 ? KEEP : 1][8];
    float part = 0.f;
#pragma unroll
    for (int n = 0; n < KEEP; ++n) {
      const int t = lane + 64 * n;
      if (t < p.items) part += ffm_item<K>(l, S, p.Q, a.F, t, Gk[n]);
    }
    for (int t = lane + 64 * KEEP; t < p.items; t += 64) {
      float G[8];
      part += ffm_item<K>(l, S, p.Q, a.F, t, G);
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
      if (t < p.items) ffm_store_item(p, l, b, t, coef, Gk[n]);
    }
    for (int t = lane + 64 * KEEP; t < p.items; t += 64) {
      float G[8];
      ffm_item<K>(l, S, p.Q, a.F, t, G);
      ffm_store_item(p, l, b, t, coef, G);
    }
    if (lane == 0) ffm_row_done(a, b, y, m, coef, loss_acc, corr_acc, cnt);
    wave_lds_sync();
  }
  if (kBwd && a.metrics) ffm_metrics(a, loss_acc, corr_acc, cnt);
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
