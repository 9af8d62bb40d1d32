// Field-weighted factorization machine on CSR rows with a field per occurrence (libffm's
// field:index:value rows, what the device text parsers emit): rows of any width, fields
// missing, repeated and in any order. One kernel for every width: a row's state is P [F, D],
// bounded whatever the row holds, so a wave walks its row in rounds of 64 occurrences and a
// row of n costs O(n D + F^2 D).
//
//   P[f]    = sum_{valid p: f_p = f} x_p v_p     q_f = sum x_p^2 |v_p|^2     n_f = count
//   R0      = R read as symmetric from its upper triangle, diagonal 0;   rd_f = R[f][f]
//   T0      = R0 P
//   s_f     = n_f >= 2 ? 1/2 (|P[f]|^2 - q_f) : 0          (selected, not masked by a product)
//           = sum_{p < p' in f} x_p x_p' <v_p, v_p'>, which is how it is summed here: position
//             p' adds <x_p' v_p', P[f] so far>. No q_f, no subtraction: on a field of 65
//             positions the fp32 chains of |P[f]|^2 and q_f left 1.6e-5 of max |dR| in
//             dR[f][f] where the test allows 4.3e-6; the pair sum has nothing to cancel.
//   m       = lin + 1/2 sum_f <P[f], T0[f]> + sum_f rd_f s_f
//   dX0[p]  = c x_p (T0[f_p] + (n_{f_p} >= 2 ? rd_{f_p} (P[f_p] - x_p v_p) : 0))
//   dR[f,g] = sum_b c_b <P_b[f], P_b[g]> (f != g),    dR[f,f] = sum_b c_b s_bf
//
// An occurrence whose field is outside [0, F) keeps its linear term w x, takes part in no pair
// and gets a zero dX0 row (ffm_csr.hip's rule). A field may repeat in one row and not in the
// next, so whether the diagonal of R acts is decided per row: it is kept out of the matrix
// product, and a field that occurs once in a row adds exactly 0 to m, dX0 and dR[f][f].
//
// * Block: R0 padded to [Fp][Fp] (Fp = F rounded up to 16) and rd [Fp] go to LDS once. One
//   wavefront per row on its own LDS region, grid-stride over B, up to four waves a block.
// * Pass 1, per round: lane j stages occurrence j of the round into the wave's tile [64][Q]
//   (ffm_src / ffm_stage), x beside it (0 for an invalid field, w x kept in a register), and
//   writes row_of. The round's field lists are rebuilt in registers by ffm_csr.hip's ballot
//   counting sort; lane f adds the round's count to n_f. Item (field f, chunk c) belongs to
//   one lane, which walks f's list in position order and carries P[f][8c..8c+7] and its share
//   of s_f through LDS from round to round: one writer per cell, one sum chain in ascending
//   position order, no LDS atomics. P rows are D + 4 floats apart, as in fwfm.hip.
// * T0 = R0 P on v_mfma_f32_16x16x4_f32 with fwfm.hip's fragments (M = Fp, N = D, K = F
//   rounded up to 4); <P, T0> comes straight from the accumulators. Lane f adds the shares of
//   s_f, by select on n_f >= 2, and leaves n_f >= 2 ? rd_f : 0 in LDS for pass 2.
// * Pass 2 (training form): rounds of 64 again. A row of n <= 64 still has its tile in LDS;
//   a wider row stages every round a second time. Item (i, c) leaves as one 16-B store.
// * dR: the upper-triangle 16 x 16 tiles of sum_b (c_b P_b) P_b^T stay in MFMA accumulators
//   across the wave's rows, once per row whatever its width; their diagonal entries are not
//   used, lane f keeps sum_b c_b s_bf in a register. The waves add both into one LDS copy in
//   wave order and the block writes dR_part[blockIdx.x] in fwfm.hip's layout (fwfm_dr_reduce
//   reads it unchanged): idle waves and blocks add zeros, no float atomics anywhere.
//
// An empty row runs one round of nothing: m = 0, it is counted. kBwd = false writes
// margins[B] and nothing else.
#include "ffm_tile.cuh"
#include "fwfm.h"

#include <algorithm>
#include <stdexcept>
#include <string>

namespace psamd {

namespace {

typedef float f32x4 __attribute__((ext_vector_type(4)));

constexpr int kSelChunks = 16;  // n_f >= 2 ? rd_f : 0, 64 floats

struct FwfmCsrK {
  FwfmCsr a;
  int C, Q, PS;     // 16-B chunks of a row, the tile's row stride (odd), floats between P rows
  int wave_chunks;  // a wave's LDS region
};

__device__ __forceinline__ f32x4 mfma4(float x, float y, f32x4 c) {
  return __builtin_amdgcn_mfma_f32_16x16x4f32(x, y, c, 0, 0, 0);
}

// row b's positions [lo, lo + n), both ends clamped to nnz (as ffm_csr_row)
__device__ __forceinline__ int fwfm_csr_row(const FwfmCsr& a, int64_t b, int64_t& lo) {
  lo = a.row_ptr[b];
  int64_t hi = a.row_ptr[b + 1];
  lo = lo < 0 ? 0 : (lo > a.nnz ? a.nnz : lo);
  hi = hi < lo ? lo : (hi > a.nnz ? a.nnz : hi);
  return (int)(hi - lo);  // nnz < 2^31
}

// Lane j < cnt stages occurrence p0 + j into the tile: the row, x (0 for a field outside
// [0, F)) and the field byte (0 then). Returns the field, -1 for none; adds w x to lin.
__device__ __forceinline__ int fwfm_csr_stage(const FwfmCsrK& p, const FfmLds& l, uint8_t* map,
                                              int64_t p0, int cnt, int lane, float& lin) {
  int f = -1;
  if (lane < cnt) {
    float x, w;
    bool ok;
    const uint4* src = ffm_src(p.a, p0 + lane, x, w, ok);
    ffm_stage(src, ok, l.tile + lane * p.Q, p.C);
    lin = fmaf(w, x, lin);
    f = p.a.fld[p0 + lane];
    if (!in_range(f, p.a.F)) f = -1, x = 0.f;
    l.xs[lane] = x;
    map[lane] = (uint8_t)(f < 0 ? 0 : f);
  }
  return f;
}

template <int NT, bool kBwd>
__global__ void __launch_bounds__(256) fwfm_csr_kernel(const FwfmCsrK p) {
  extern __shared__ uint4 smem[];
  constexpr int Fp = NT * 16, NTRI = NT * (NT + 1) / 2;
  const FwfmCsr& a = p.a;
  const int F = a.F, D = a.Dr, C = p.C, Q = p.Q, PS = p.PS;
  float* Rl = reinterpret_cast<float*>(smem);
  float* rdl = Rl + Fp * Fp;
  for (int e = threadIdx.x; e < Fp * Fp; e += blockDim.x) {
    const int f = e / Fp, g = e - f * Fp;
    const int lo = min(f, g), hi = max(f, g);
    Rl[e] = hi < F && f != g ? a.R[lo * F + hi] : 0.f;
    if (e < Fp) rdl[e] = e < F ? a.R[e * F + e] : 0.f;
  }
  __syncthreads();
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6, W = blockDim.x >> 6;
  const int i16 = lane & 15, g4 = lane >> 4;
  const uint64_t below = (1ull << lane) - 1;
  uint4* region = smem + (Fp * Fp + Fp) / 4;
  uint8_t* map = reinterpret_cast<uint8_t*>(region + wv * p.wave_chunks);
  FfmLds l;
  l.fld = map;
  l.pos = map + 64;
  l.off = map + 128;
  l.tile = reinterpret_cast<uint4*>(map) + kFfmMapChunks;
  l.xs = reinterpret_cast<float*>(l.tile + 64 * Q);
  float* P = l.xs + kFfmXsChunks * 4;
  float* sp = P + Fp * PS;
  float* T = sp + Fp * C;  // s_f shares [Fp][C]; behind them the training form's T0 and rsel
  float* rsel = T + Fp * PS;
  f32x4 acc[NTRI];
#pragma unroll
  for (int t = 0; t < NTRI; ++t) acc[t] = f32x4{0.f, 0.f, 0.f, 0.f};
  float cd = 0.f;  // lane f: sum over the wave's rows of c_b s_bf
  double loss_acc = 0, corr_acc = 0, cnt_acc = 0;
  for (int64_t b = blockIdx.x * (int64_t)W + wv; b < a.B; b += (int64_t)gridDim.x * W) {
    int64_t lo;
    const int n = fwfm_csr_row(a, b, lo);
    float lin = 0.f;
    int nf = 0;  // lane f: occurrences of field f in the row
    // ---- pass 1: the field sums P [Fp][D] and the shares of q_f, round by round
    for (int base = 0; base == 0 || base < n; base += 64) {
      const int cnt = min(64, n - base);
      const int f = fwfm_csr_stage(p, l, map, lo + base, cnt, lane, lin);
      if (kBwd && lane < cnt) a.row_of[lo + base + lane] = (int32_t)b;
      // counting sort by field: rank among earlier lanes of the same field, counts by field
      int rank = 0, mine = 0;
      for (uint64_t todo = __ballot(f >= 0); todo;) {
        const int fs = __builtin_amdgcn_readlane(f, __ffsll((unsigned long long)todo) - 1);
        const uint64_t same = __ballot(f == fs);
        if (f == fs) rank = __popcll(same & below);
        if (lane == fs) mine = __popcll(same);
        todo &= ~same;
      }
      nf += mine;
      int incl = mine;
#pragma unroll
      for (int d = 1; d < 64; d <<= 1) {
        const int up = __shfl_up(incl, d, 64);
        if (lane >= d) incl += up;
      }
      const int first = __shfl(incl - mine, f < 0 ? 0 : f, 64);  // off[f]
      map[128 + 1 + lane] = (uint8_t)incl;
      if (lane == 0) map[128] = 0;
      if (f >= 0) map[64 + first + rank] = (uint8_t)lane;
      wave_lds_sync();
      for (int t = lane; t < Fp * C; t += 64) {
        const int c = t / Fp, fi = t - c * Fp;
        float4* dst = reinterpret_cast<float4*>(P + fi * PS + c * 8);
        float s[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
        float ss = 0.f;
        if (base) {  // the cell's own earlier rounds: one chain over the whole row
          const float4 s0 = dst[0], s1 = dst[1];
          s[0] = s0.x, s[1] = s0.y, s[2] = s0.z, s[3] = s0.w;
          s[4] = s1.x, s[5] = s1.y, s[6] = s1.z, s[7] = s1.w;
          ss = sp[fi * C + c];
        }
        const int q1 = l.off[fi + 1];
        for (int q = l.off[fi]; q < q1; ++q) {
          const int j = l.pos[q];
          const float x = l.xs[j];
          const uint4 v = l.tile[j * Q + c];
          const uint32_t vw[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
          for (int e = 0; e < 4; ++e) {
            const float vl = x * __uint_as_float(vw[e] << 16);
            const float vh = x * __uint_as_float(vw[e] & 0xffff0000u);
            ss = fmaf(vl, s[2 * e], ss);  // against the positions before this one
            ss = fmaf(vh, s[2 * e + 1], ss);
            s[2 * e] += vl;
            s[2 * e + 1] += vh;
          }
        }
        dst[0] = make_float4(s[0], s[1], s[2], s[3]);
        dst[1] = make_float4(s[4], s[5], s[6], s[7]);
        sp[fi * C + c] = ss;
      }
      wave_lds_sync();  // P is written; the next round's stage writes what this one read
    }
    // ---- T0 = R0 P on the matrix cores; <P, T0> straight from the accumulators
    float part = 0.f;
    const int K4 = (F + 3) >> 2;
    for (int n0 = 0; n0 < D; n0 += 16) {
      const int nn = n0 + i16;
      const bool nok = nn < D;
      f32x4 t[NT];
#pragma unroll
      for (int mt = 0; mt < NT; ++mt) t[mt] = f32x4{0.f, 0.f, 0.f, 0.f};
      for (int kk = 0; kk < K4; ++kk) {
        const int k = kk * 4 + g4;
        const float bv = nok ? P[k * PS + nn] : 0.f;
#pragma unroll
        for (int mt = 0; mt < NT; ++mt) t[mt] = mfma4(Rl[k * Fp + mt * 16 + i16], bv, t[mt]);
      }
      if (nok) {
#pragma unroll
        for (int mt = 0; mt < NT; ++mt)
#pragma unroll
          for (int r = 0; r < 4; ++r) {
            const int fi = mt * 16 + 4 * g4 + r;
            if (kBwd) T[fi * PS + nn] = t[mt][r];
            part = fmaf(t[mt][r], P[fi * PS + nn], part);
          }
      }
    }
    // ---- the diagonal: lane f, by select on n_f >= 2
    float sf = 0.f, rds = 0.f;
    if (lane < F && nf >= 2) {
      for (int c = 0; c < C; ++c) sf += sp[lane * C + c];
      rds = rdl[lane];
    }
    const float m = wave_allsum(lin + 0.5f * part + rds * sf);
    if (!kBwd) {
      if (lane == 0) a.margins[b] = m;
      wave_lds_sync();  // the next row's stage writes what this one read
      continue;
    }
    const float y = a.labels[b] > 0.f ? 1.f : -1.f;
    const float coef = -y / (1.f + expf(y * m));
    cd = fmaf(coef, sf, cd);
    rsel[lane] = rds;
    wave_lds_sync();  // T0 and rsel are written
    // ---- pass 2: dX0[i][c] = c x_i (T0[f_i][c] + rsel[f_i] (P[f_i][c] - x_i v_i[c]))
    for (int base = 0; base < n; base += 64) {
      const int cnt = min(64, n - base);
      if (n > 64) {  // a narrower row's tile is still pass 1's
        wave_lds_sync();
        float unused = 0.f;
        fwfm_csr_stage(p, l, map, lo + base, cnt, lane, unused);
        wave_lds_sync();
      }
      for (int t = lane; t < cnt * C; t += 64) {
        const int c = t / cnt, i = t - c * cnt;
        const int fi = l.fld[i];
        const float x = l.xs[i], rs = rsel[fi];
        const uint4 v = l.tile[i * Q + c];
        const uint32_t vw[4] = {v.x, v.y, v.z, v.w};
        const float4* tp = reinterpret_cast<const float4*>(T + fi * PS + c * 8);
        const float4* pp = reinterpret_cast<const float4*>(P + fi * PS + c * 8);
        const float4 t0 = tp[0], t1 = tp[1], p0 = pp[0], p1 = pp[1];
        const float tv[8] = {t0.x, t0.y, t0.z, t0.w, t1.x, t1.y, t1.z, t1.w};
        const float pv[8] = {p0.x, p0.y, p0.z, p0.w, p1.x, p1.y, p1.z, p1.w};
        float G[8];
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          const float vl = __uint_as_float(vw[e] << 16), vh = __uint_as_float(vw[e] & 0xffff0000u);
          G[2 * e] = fmaf(rs, fmaf(-x, vl, pv[2 * e]), tv[2 * e]);
          G[2 * e + 1] = fmaf(rs, fmaf(-x, vh, pv[2 * e + 1]), tv[2 * e + 1]);
        }
        ffm_store(a.dX0, lo + base + i, D, c, coef * x, G);
      }
    }
    // ---- dR tiles += (c P) P^T, K = D
    for (int kk = 0; kk < D; kk += 4) {
      float fr[NT];
#pragma unroll
      for (int t = 0; t < NT; ++t) fr[t] = P[(t * 16 + i16) * PS + kk + g4];
      int u = 0;
#pragma unroll
      for (int t1 = 0; t1 < NT; ++t1) {
        const float av = coef * fr[t1];
#pragma unroll
        for (int t2 = t1; t2 < NT; ++t2, ++u) acc[u] = mfma4(av, fr[t2], acc[u]);
      }
    }
    if (lane == 0) ffm_row_done(a, b, y, m, coef, loss_acc, corr_acc, cnt_acc);
    wave_lds_sync();
  }
  if (!kBwd) return;
  if (a.metrics) ffm_metrics(a, loss_acc, corr_acc, cnt_acc);
  // ---- the block's partial: zero, then the waves' tiles and diagonals in wave order, in
  // the LDS the regions and rd held
  __syncthreads();
  float* dRl = reinterpret_cast<float*>(region);
  for (int e = threadIdx.x; e < Fp * Fp; e += blockDim.x) {
    dRl[e] = 0.f;
    if (e < Fp) rdl[e] = 0.f;
  }
  __syncthreads();
  for (int w = 0; w < W; ++w) {
    if (wv == w) {
      int u = 0;
#pragma unroll
      for (int t1 = 0; t1 < NT; ++t1)
#pragma unroll
        for (int t2 = t1; t2 < NT; ++t2, ++u)
#pragma unroll
          for (int r = 0; r < 4; ++r)
            dRl[(t1 * 16 + 4 * g4 + r) * Fp + t2 * 16 + i16] += acc[u][r];
      if (lane < F) rdl[lane] += cd;
    }
    __syncthreads();
  }
  float* out = a.dR_part + (int64_t)blockIdx.x * (Fp * Fp);
  for (int e = threadIdx.x; e < Fp * Fp; e += blockDim.x) {
    const int f = e / Fp, g = e - f * Fp;
    out[e] = f != g ? dRl[e] : rdl[f];
  }
}

template <bool kBwd>
void fwfm_csr_launch(const FwfmCsr& a, hipStream_t st) {
  auto bad = [](const std::string& s) { throw std::invalid_argument("fwfm_csr: " + s); };
  if (a.F < 1 || a.F > 64) bad("1..64 fields, not " + std::to_string(a.F));
  if (a.Dr != 8 && a.Dr != 16 && a.Dr != 32) bad("D in {8, 16, 32}, not " + std::to_string(a.Dr));
  if (a.nnz < 0 || a.nnz >= (int64_t(1) << 31)) bad("0 <= nnz < 2^31");
  if (!a.row_ptr || (a.nnz > 0 && !a.fld)) bad("no row_ptr / fld");
  if (!a.R) bad("no R");
  if (kBwd && (!a.dR_part || a.parts < 1 || a.parts > 4096))
    bad("1..4096 dR partials, not " + std::to_string(a.parts));
  if (kBwd && a.nnz > 0 && !a.row_of) bad("no row_of");
  if (a.B <= 0 && !kBwd) return;
  FwfmCsrK p = {};
  p.a = a;
  p.C = a.Dr / 8;
  p.Q = p.C | 1;
  p.PS = a.Dr + 4;
  const int NT = (a.F + 15) / 16, Fp = NT * 16;
  p.wave_chunks = kFfmMapChunks + 64 * p.Q + kFfmXsChunks + Fp * p.PS / 4 + Fp * p.C / 4 +
                  (kBwd ? Fp * p.PS / 4 + kSelChunks : 0);
  // as many waves (rows) per block as 64 KB of LDS hold beside R0 and rd, four at the most;
  // the block's dR copy reuses the waves' regions
  const int head = (Fp * Fp + Fp) * 4, wave_bytes = p.wave_chunks * 16;
  const int W = std::min(4, (65536 - head) / wave_bytes);
  const size_t lds = head + std::max<size_t>((size_t)W * wave_bytes, kBwd ? Fp * Fp * 4 : 0);
  // the training form launches one block per partial, whatever B is: the reduce reads all
  const unsigned g = kBwd ? (unsigned)a.parts
                          : (unsigned)std::min<int64_t>((a.B + 2 * W - 1) / (2 * W), 1 << 16);
#define PSAMD_FWFM_CSR(N) \
  if (NT == N) fwfm_csr_kernel<N, kBwd><<<g, 64 * W, lds, st>>>(p)
  PSAMD_FWFM_CSR(1);
  PSAMD_FWFM_CSR(2);
  PSAMD_FWFM_CSR(3);
  PSAMD_FWFM_CSR(4);
#undef PSAMD_FWFM_CSR
  PSAMD_HIP_CHECK(hipGetLastError());
}

}  // namespace

void fwfm_csr_fwd_bwd(const FwfmCsr& a, hipStream_t st) { fwfm_csr_launch<true>(a, st); }
void fwfm_csr_margins(const FwfmCsr& a, hipStream_t st) { fwfm_csr_launch<false>(a, st); }

}  // namespace psamd
