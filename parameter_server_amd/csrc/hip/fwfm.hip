// Field-weighted factorization machine (FwFM, Pan et al. 2018): fused forward + backward on
// rows of a fixed width S <= 64, one wavefront per example, the two small matrix products of
// a row on the fp32 matrix instructions.
//
//   m        = sum_i x_i w_i + sum_{i<j} x_i x_j R[f_i][f_j] <v_i, v_j>
//   P[f]     = sum_{i: f_i = f} x_i v_i          [F, D]      q_f = sum_{i: f_i = f} x_i^2 |v_i|^2
//   T        = R P                               [F, D]
//   m        = lin + 1/2 (sum_f <P[f], T[f]> - sum_f R[f][f] q_f)
//   dX0[i]   = c x_i (T[f_i] - R[f_i][f_i] x_i v_i),   c = -y sigma(-y m)
//   dR[f,g]  = sum_b c_b <P_b[f], P_b[g]>  (f < g),    dR[f,f] = 1/2 sum_b c_b (|P_b[f]|^2 - q_bf)
//
// A key owns one vector of D bf16, as in the FM; the field pair strengths R [F, F] are a small
// dense parameter, read as symmetric. Neither the FM's |sum v|^2 identity nor the FFM's pair
// walk applies: a row costs O(S D + F^2 D), and every factor row is read once.
//
// * Block: the field lists (ffm.hip's packed bytes) and R, symmetrised from its upper
//   triangle and zero-padded to [Fp][Fp], Fp = F rounded up to 16, go to LDS once; the
//   diagonal entry of a field with fewer than two positions (no same-field pair) is read
//   as 0. Two barriers, then every wave works on its own LDS region, grid-stride over B.
// * Stage: ffm_src / ffm_stage of ffm_tile.cuh, unchanged: lane j < S loads row j into the
//   wave's tile [S][Q] of 16-B chunks (Q = D / 8 made odd), x_j beside it.
// * Field sums: item (field f < Fp, chunk c) belongs to one lane, which walks f's positions
//   in list order and writes 8 fp32 of P[f] and its share of q_f: one writer per cell, a
//   fixed sum order, no LDS atomics. Rows F..Fp-1 have empty lists and come out zero. P rows
//   are D + 4 floats apart: the fragment reads below (16 rows x 4 columns) then touch every
//   bank twice, the least 64 lanes can.
// * T = R P: v_mfma_f32_16x16x4_f32, M = Fp (NT tiles, all in flight on one B fragment),
//   N = D (one or two tiles; D = 8 masks half a tile), K = F rounded up to 4. A comes from
//   the LDS copy of R (read transposed, R is symmetric: 16 consecutive floats per k), B from
//   P. The accumulators go to T in LDS (the lane of position i needs row f_i) and, times the
//   matching P cell, into the margin, so the margin needs no second pass.
// * dX0[i][c] leaves as one 16-B store by the lane of item (i, c), as the FFM's.
// * dR: the wave keeps the upper-triangle 16 x 16 tiles of sum_b (c_b P_b) P_b^T in MFMA
//   accumulators across all its rows (NT (NT + 1) / 2 tiles of 4 registers); A and B are
//   the same fragment of P, A scaled by c_b, K = D. The -q_f of the diagonal is a VALU sum
//   in lane f. After the row loop the waves add their tiles into one LDS copy in wave order
//   and the block writes it to dR_part[blockIdx.x]: idle waves and blocks add zeros, no
//   float atomics anywhere. fwfm_dr_reduce_kernel sums the partials in a fixed order,
//   mirrors, and applies AdaGrad to R when asked.
//
// kBwd = false writes margins[B] and nothing else (no accumulators, no T in LDS).
#include "ffm_tile.cuh"
#include "fwfm.h"

#include <algorithm>
#include <stdexcept>
#include <string>

namespace psamd {

namespace {

typedef float f32x4 __attribute__((ext_vector_type(4)));

constexpr int kMapWords = 49;  // bytes: fld[64] | pos[64] | off[65 -> 68], as ffm.hip
constexpr int kMapChunks = kFfmMapChunks;
constexpr int kXsChunks = kFfmXsChunks;
constexpr int kQpChunks = 64;  // q_f shares [Fp][C] <= 256 floats

struct FwfmK {
  Fwfm a;
  int C, Q, PS;     // 16-B chunks of a row, the tile's row stride (odd), floats between P rows
  int wave_chunks;  // a wave's LDS region
  uint32_t map[kMapWords];
};

__device__ __forceinline__ f32x4 mfma4(float x, float y, f32x4 c) {
  return __builtin_amdgcn_mfma_f32_16x16x4f32(x, y, c, 0, 0, 0);
}

template <int NT, bool kBwd>
__global__ void __launch_bounds__(256) fwfm_kernel(const FwfmK p) {
  extern __shared__ uint4 smem[];
  constexpr int Fp = NT * 16, NTRI = NT * (NT + 1) / 2;
  const Fwfm& a = p.a;
  const int S = a.S, F = a.F, D = a.Dr, C = p.C, Q = p.Q, PS = p.PS;
  float* Rl = reinterpret_cast<float*>(smem + kMapChunks);
  if (threadIdx.x == 0) {
    uint32_t* mw = reinterpret_cast<uint32_t*>(smem);
#pragma unroll
    for (int w = 0; w < kMapWords; ++w) mw[w] = p.map[w];
  }
  __syncthreads();
  // a field of fewer than two positions has no same-field pair, so its diagonal entry has no
  // part in the model: it is read as 0, and T[f] - R[f][f] x v needs no cancellation there
  const uint8_t* off = reinterpret_cast<const uint8_t*>(smem) + 128;
  for (int e = threadIdx.x; e < Fp * Fp; e += blockDim.x) {
    const int f = e / Fp, g = e - f * Fp;
    const int lo = min(f, g), hi = max(f, g);
    Rl[e] = hi < F && (f != g || off[f + 1] - off[f] >= 2) ? a.R[lo * F + hi] : 0.f;
  }
  __syncthreads();
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6, W = blockDim.x >> 6;
  const int i16 = lane & 15, g4 = lane >> 4;
  uint4* region = smem + kMapChunks + Fp * Fp / 4;
  FfmLds l;
  l.fld = reinterpret_cast<const uint8_t*>(smem);
  l.pos = l.fld + 64;
  l.off = l.fld + 128;
  l.tile = region + wv * p.wave_chunks;
  l.xs = reinterpret_cast<float*>(l.tile + S * Q);
  float* P = l.xs + kXsChunks * 4;
  float* T = P + Fp * PS;
  float* qp = T + Fp * PS;
  f32x4 acc[NTRI];
#pragma unroll
  for (int t = 0; t < NTRI; ++t) acc[t] = f32x4{0.f, 0.f, 0.f, 0.f};
  float cq = 0.f;  // lane f: sum over the wave's rows of c_b q_bf
  double loss_acc = 0, corr_acc = 0, cnt = 0;
  for (int64_t b = blockIdx.x * (int64_t)W + wv; b < a.B; b += (int64_t)gridDim.x * W) {
    float lin = 0.f;
    if (lane < S) {
      float x, w;
      bool ok;
      const uint4* src = ffm_src(a, b * S + lane, x, w, ok);
      ffm_stage(src, ok, l.tile + lane * Q, C);
      l.xs[lane] = x;
      lin = w * x;
    }
    wave_lds_sync();
    // ---- field sums: P [Fp][D] and the shares of q_f
    for (int t = lane; t < Fp * C; t += 64) {
      const int c = t / Fp, f = t - c * Fp;
      float s[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
      float qq = 0.f;
      const int q1 = l.off[f + 1];
      for (int q = l.off[f]; q < q1; ++q) {
        const int j = l.pos[q];
        const float x = l.xs[j];
        const uint4 v = l.tile[j * Q + c];
        const uint32_t vw[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          const float lo = x * __uint_as_float(vw[e] << 16);
          const float hi = x * __uint_as_float(vw[e] & 0xffff0000u);
          s[2 * e] += lo;
          s[2 * e + 1] += hi;
          qq = fmaf(lo, lo, qq);
          qq = fmaf(hi, hi, qq);
        }
      }
      float4* dst = reinterpret_cast<float4*>(P + f * PS + c * 8);
      dst[0] = make_float4(s[0], s[1], s[2], s[3]);
      dst[1] = make_float4(s[4], s[5], s[6], s[7]);
      qp[f * C + c] = qq;
    }
    wave_lds_sync();
    // ---- T = R P on the matrix cores; <P, T> straight from the accumulators
    float part = 0.f;
    const int K4 = (F + 3) >> 2;
    for (int n0 = 0; n0 < D; n0 += 16) {
      const int n = n0 + i16;
      const bool nok = n < D;
      f32x4 t[NT];
#pragma unroll
      for (int mt = 0; mt < NT; ++mt) t[mt] = f32x4{0.f, 0.f, 0.f, 0.f};
      for (int kk = 0; kk < K4; ++kk) {
        const int k = kk * 4 + g4;
        const float bv = nok ? P[k * PS + n] : 0.f;
#pragma unroll
        for (int mt = 0; mt < NT; ++mt) t[mt] = mfma4(Rl[k * Fp + mt * 16 + i16], bv, t[mt]);
      }
      if (nok) {
#pragma unroll
        for (int mt = 0; mt < NT; ++mt)
#pragma unroll
          for (int r = 0; r < 4; ++r) {
            const int f = mt * 16 + 4 * g4 + r;
            if (kBwd) T[f * PS + n] = t[mt][r];
            part = fmaf(t[mt][r], P[f * PS + n], part);
          }
      }
    }
    float qf = 0.f, rq = 0.f;
    if (lane < F) {
      for (int c = 0; c < C; ++c) qf += qp[lane * C + c];
      rq = Rl[lane * Fp + lane] * qf;
    }
    const float m = wave_allsum(lin + 0.5f * (part - rq));
    if (!kBwd) {
      if (lane == 0) a.margins[b] = m;
      wave_lds_sync();  // the next row's stage writes what this one read
      continue;
    }
    const float y = a.labels[b] > 0.f ? 1.f : -1.f;
    const float coef = -y / (1.f + expf(y * m));
    cq = fmaf(coef, qf, cq);
    wave_lds_sync();  // T is written
    // ---- dX0[i][c] = c x_i (T[f_i][c] - R[f_i][f_i] x_i v_i[c])
    for (int t = lane; t < S * C; t += 64) {
      const int c = t / S, i = t - c * S;
      const int f = l.fld[i];
      const float x = l.xs[i];
      const float rd = Rl[f * Fp + f] * x;
      const uint4 v = l.tile[i * Q + c];
      const uint32_t vw[4] = {v.x, v.y, v.z, v.w};
      const float4* tp = reinterpret_cast<const float4*>(T + f * PS + c * 8);
      const float4 t0 = tp[0], t1 = tp[1];
      const float tv[8] = {t0.x, t0.y, t0.z, t0.w, t1.x, t1.y, t1.z, t1.w};
      float G[8];
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        G[2 * e] = fmaf(-rd, __uint_as_float(vw[e] << 16), tv[2 * e]);
        G[2 * e + 1] = fmaf(-rd, __uint_as_float(vw[e] & 0xffff0000u), tv[2 * e + 1]);
      }
      ffm_store(a.dX0, b * S + i, D, c, coef * x, G);
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
    if (lane == 0) ffm_row_done(a, b, y, m, coef, loss_acc, corr_acc, cnt);
    wave_lds_sync();
  }
  if (!kBwd) return;
  if (a.metrics) ffm_metrics(a, loss_acc, corr_acc, cnt);
  // ---- the block's partial: zero, then the waves' tiles in wave order, in the LDS the
  // regions held
  __syncthreads();
  float* dRl = reinterpret_cast<float*>(region);
  for (int e = threadIdx.x; e < Fp * Fp; e += blockDim.x) dRl[e] = 0.f;
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
      wave_lds_sync();
      if (lane < F) dRl[lane * Fp + lane] -= cq;
    }
    __syncthreads();
  }
  float* out = a.dR_part + (int64_t)blockIdx.x * (Fp * Fp);
  for (int e = threadIdx.x; e < Fp * Fp; e += blockDim.x) {
    const int f = e / Fp, g = e - f * Fp;
    // a field of fewer than two positions has no same-field pair: its diagonal entry is 0
    // by construction (|P[f]|^2 = q_f), not whatever the two roundings leave
    out[e] = f != g ? dRl[e] : (l.off[f + 1] - l.off[f] >= 2 ? 0.5f * dRl[e] : 0.f);
  }
}

__global__ void __launch_bounds__(256) fwfm_dr_reduce_kernel(const FwfmReduce a, int Fp) {
  __shared__ float sl[16][17];
  const int e = threadIdx.x & 15, s = threadIdx.x >> 4;
  const int id = blockIdx.x * 16 + e, F = a.F;
  const int f = id / F, g = id - f * F;
  const bool mine = id < F * F && f <= g;  // the upper triangle works, and writes both halves
  float v = 0.f;
  if (mine && a.sum) {
    const int per = (a.parts + 15) / 16;
    const int b1 = min(a.parts, (s + 1) * per);
    const float* src = a.dR_part + f * Fp + g;
    for (int b = s * per; b < b1; ++b) v += src[(int64_t)b * (Fp * Fp)];
  }
  sl[s][e] = v;
  __syncthreads();
  if (s != 0 || !mine) return;
  float d = 0.f;
  if (a.sum) {
#pragma unroll
    for (int s2 = 0; s2 < 16; ++s2) d += sl[s2][e];
    a.dR[f * F + g] = d;
    a.dR[g * F + f] = d;
  } else {
    d = a.dR[f * F + g];
  }
  if (a.update) {
    float r = a.R[f * F + g];
    const float gr = fmaf(a.lambda_r, r, d);
    const float ac = fmaf(gr, gr, a.acc[f * F + g]);
    r -= a.lr * gr / (sqrtf(ac) + 1e-8f);
    a.acc[f * F + g] = ac;
    a.acc[g * F + f] = ac;
    a.R[f * F + g] = r;
    a.R[g * F + f] = r;
  }
}

template <bool kBwd>
void fwfm_launch(const Fwfm& a, hipStream_t st) {
  auto bad = [](const std::string& s) { throw std::invalid_argument("fwfm: " + s); };
  if (a.S < 1 || a.S > 64) bad("1..64 positions per row, not " + std::to_string(a.S));
  if (a.F < 1 || a.F > 64) bad("1..64 fields, not " + std::to_string(a.F));
  if (a.Dr != 8 && a.Dr != 16 && a.Dr != 32) bad("D in {8, 16, 32}, not " + std::to_string(a.Dr));
  if (!a.fields) bad("no field map");
  for (int i = 0; i < a.S; ++i)
    if (a.fields[i] < 0 || a.fields[i] >= a.F)
      bad("field " + std::to_string(a.fields[i]) + " of position " + std::to_string(i) +
          " outside [0, " + std::to_string(a.F) + ")");
  if (!a.R) bad("no R");
  if (kBwd && (!a.dR_part || a.parts < 1 || a.parts > 4096))
    bad("1..4096 dR partials, not " + std::to_string(a.parts));
  if (a.B <= 0 && !kBwd) return;
  FwfmK p = {};
  p.a = a;
  p.a.fields = nullptr;
  p.C = a.Dr / 8;
  p.Q = p.C | 1;
  p.PS = a.Dr + 4;
  uint8_t* mb = reinterpret_cast<uint8_t*>(p.map);  // fld | pos | off, positions in row order
  int n = 0;
  for (int f = 0; f < a.F; ++f) {
    mb[128 + f] = (uint8_t)n;
    for (int i = 0; i < a.S; ++i)
      if (a.fields[i] == f) mb[64 + n++] = (uint8_t)i;
  }
  for (int f = a.F; f <= 64; ++f) mb[128 + f] = (uint8_t)n;
  for (int i = 0; i < a.S; ++i) mb[i] = (uint8_t)a.fields[i];
  const int NT = (a.F + 15) / 16, Fp = NT * 16;
  p.wave_chunks = a.S * p.Q + kXsChunks + 2 * (Fp * p.PS / 4) + kQpChunks;
  // as many waves (rows) per block as 64 KB of LDS hold beside the map and R, four at the
  // most; the block's dR copy reuses the waves' regions
  const int head = kMapChunks * 16 + Fp * Fp * 4, wave_bytes = p.wave_chunks * 16;
  const int W = std::min(4, (65536 - head) / wave_bytes);
  const size_t lds = head + std::max<size_t>((size_t)W * wave_bytes, kBwd ? Fp * Fp * 4 : 0);
  // the training form launches one block per partial, whatever B is: the reduce reads all
  const unsigned g = kBwd ? (unsigned)a.parts
                          : (unsigned)std::min<int64_t>((a.B + 2 * W - 1) / (2 * W), 1 << 16);
#define PSAMD_FWFM(N) \
  if (NT == N) fwfm_kernel<N, kBwd><<<g, 64 * W, lds, st>>>(p)
  PSAMD_FWFM(1);
  PSAMD_FWFM(2);
  PSAMD_FWFM(3);
  PSAMD_FWFM(4);
#undef PSAMD_FWFM
  PSAMD_HIP_CHECK(hipGetLastError());
}

}  // namespace

void fwfm_fwd_bwd(const Fwfm& a, hipStream_t st) { fwfm_launch<true>(a, st); }
void fwfm_margins(const Fwfm& a, hipStream_t st) { fwfm_launch<false>(a, st); }

void fwfm_dr_reduce(const FwfmReduce& a, hipStream_t st) {
  auto bad = [](const std::string& s) { throw std::invalid_argument("fwfm_dr_reduce: " + s); };
  if (a.F < 1 || a.F > 64) bad("1..64 fields, not " + std::to_string(a.F));
  if (!a.sum && !a.update) bad("nothing to do");
  if (!a.dR) bad("no dR");
  if (a.sum && (!a.dR_part || a.parts < 1 || a.parts > 4096))
    bad("1..4096 dR partials, not " + std::to_string(a.parts));
  if (a.update && (!a.R || !a.acc)) bad("the update needs R and its accumulator");
  const int Fp = (a.F + 15) / 16 * 16;
  fwfm_dr_reduce_kernel<<<(a.F * a.F + 15) / 16, 256, 0, st>>>(a, Fp);
  PSAMD_HIP_CHECK(hipGetLastError());
}

}  // namespace psamd
