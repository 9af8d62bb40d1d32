// Scoring a minibatch against a stored field-weighted factorization machine: margins, loss /
// accuracy sums and the bucketed-AUC histogram in ONE launch, straight from the raw keys, the
// KV table, the bf16 factor rows at the slot index of every key (EmbeddingShard.rows) and
// R [F, F], for rows of any width. The model and its rules are fwfm_csr.hip's:
//
//   P[f]  = sum_{valid p: f_p = f} x_p v_p          n_f = count of valid p in f
//   s_f   = n_f >= 2 ? sum_{p < p' in f} x_p x_p' <v_p, v_p'> : 0     (selected, not multiplied)
//   m     = sum_p x_p w_p + sum_{f<g} R[f][g] <P[f], P[g]> + sum_f R[f][f] s_f
//
// R is read as symmetric from its upper triangle; an absent key contributes nothing; a field
// outside [0, F) keeps its linear term and enters no pair; a key that occurs twice is two
// positions; a field that occurs once in a row adds exactly 0 through the diagonal.
//
// Where fwfm_csr_kernel<NT, false> stages a [64][Q] bf16 tile per wave and multiplies T0 = R0 P,
// a forward-only pass reads every factor row once and needs nothing of T: here the field
// sums are built straight from global memory and the pair sum is sum Ru o (P P^T).
//
// * Block: Ru [Fp][Fp + 4] (Ru[f][g] = f < g < F ? R[f][g] : 0; Fp = F rounded up to 16; the
//   4 floats of padding put the four row groups of an accumulator read on separate banks) and
//   rd [Fp] go to LDS once. One wavefront per row, grid-stride over B, on a per-wave region
//     P f32 [Fp][D + 4] | sp f32 [Fp][C] | slot int32 [64] | x f32 [64] | pos bytes [64] |
//     off bytes [Fp + 1]
//   (C = D / 8 chunks of 16 bytes; P rows D + 4 floats apart, as in fwfm.hip: the MFMA
//   fragment reads of 16 neighbouring rows fall on 16 different banks).
//   A row runs in rounds of 64 occurrences:
// * Probe phase, lane = occurrence (ffm_predict.hip's, through probe.cuh): mix the raw key,
//   one 16-byte first-probe load per lane at a clamped address, all issued before any is
//   inspected; only a miss on an occupied slot walks its chain. lin += w x in the lane. The
//   slot and x go to LDS; a lane without a slot or with a field outside [0, F) is in no list.
// * Field lists: the ballot counting sort of ffm_csr.hip / fwfm_csr.hip in registers; lane f
//   adds the round's count to n_f.
// * Field sums, no staged tile: item (f, c) = field x chunk, item t = f C + c on lane t % 64,
//   the same dealing in every round, kGang = 2 items of a lane at a time, their loads in
//   flight together (Fp C <= 128 items but for D = 32 on more than 32 fields: one gang, and
//   half the registers of ffm_predict.hip's four). The lane walks f's list in position order, loads
//   rows[slot_j][8 c, +8) from global memory, adds <x_j v_j, P[f] so far> to its share of s_f
//   and x_j v_j to its 8 cells of P; both are carried through LDS from round to round (read
//   back in a later round, zero in the first, written once a round). One writer per cell,
//   one chain in ascending position order, no LDS atomics; s_f is the pair sum itself, never
//   1/2 (|P[f]|^2 - q_f) (fwfm_csr.hip says why).
// * Pair phase, once per row: the NT (NT + 1) / 2 upper-triangle 16 x 16 tiles of G = P P^T
//   on v_mfma_f32_16x16x4_f32 (M = N = Fp, K = D; A and B are the same fragment of P, the dR
//   scheme of fwfm.hip without the coefficient), then sum Ru o G with Ru read in the
//   accumulator's own layout: lane (i16, g4), register r <-> row 16 t1 + 4 g4 + r, column
//   16 t2 + i16. Nothing of T is ever written. F = 39, D = 16: 24 matrix instructions a row
//   (T0 = R0 P takes 36). Lane f adds rd_f s_f by select on n_f >= 2; m = wave_allsum(...).
// * Epilogue: ffm_predict_kernel's (lane 0: margin, loss terms; f64 sums by per-wave DPP;
//   the row's AUC count is one atomic add into the u64 striped global bins).
//
// Every sum has an order fixed by the row's occurrences and (F, D) alone, never by the slot a
// key sits in: a margin is the same bits on every run, for every table layout, and for a
// fixed-width row and the same row in CSR form. Read-only on the table, the rows and R; a
// slot index is used for a load only after the probe has produced it. An empty row runs no
// round: m = 0, it is counted.
#include "fwfm_predict.h"
#include "ffm_tile.cuh"
#include "loss.cuh"
#include "probe.cuh"

#include <algorithm>
#include <stdexcept>
#include <string>

namespace psamd {

namespace {

typedef float f32x4 __attribute__((ext_vector_type(4)));

constexpr int kMetaWords = 64 + 64 + 16 + 20;  // slot, x, pos bytes, off bytes (Fp + 1 <= 80)
constexpr int kGang = 2;                       // items of a lane whose loads fly together

struct FwfmPredict {
  const Slot* slots;
  uint64_t mask, home_base, home_m;
  int home_shr;
  KeyMix km;
  const uint16_t* rows;  // [mask + 1, D] bf16
  const float* R;        // [F, F]
  int D, F, cs, PS;      // C = 1 << cs chunks, PS = P's row stride in floats
  const uint64_t* keys;
  int64_t nnz;
  const int64_t* row_ptr;
  int width;
  const int32_t *fields, *field_of;
  const float* vals;
  const float* labels;
  int64_t B;
  int loss_type;
  float* margin;
  double* metrics;
  int acc_stripes;
  unsigned long long* hist;
  int nbins, hist_stripes;
  int wave_words;  // u32 words of a wave's LDS region
};

__device__ __forceinline__ f32x4 mfma4(float x, float y, f32x4 c) {
  return __builtin_amdgcn_mfma_f32_16x16x4f32(x, y, c, 0, 0, 0);
}

// One position of a field's walk, for the 8 bf16 of one chunk: ss += <x v, cells> against
// the positions before this one, then cells += x v (fwfm_csr_kernel's chain)
__device__ __forceinline__ void fwfm_cells_acc(const uint4& r, float x, float (&s)[8],
                                               float& ss) {
  const uint32_t u[4] = {r.x, r.y, r.z, r.w};
#pragma unroll
  for (int e = 0; e < 4; ++e) {  // bf16 pairs, low half first
    const float vl = x * __uint_as_float(u[e] << 16);
    const float vh = x * __uint_as_float(u[e] & 0xffff0000u);
    ss = fmaf(vl, s[2 * e], ss);
    ss = fmaf(vh, s[2 * e + 1], ss);
    s[2 * e] += vl;
    s[2 * e + 1] += vh;
  }
}

template <int NT>
__global__ void __launch_bounds__(256) fwfm_predict_kernel(const FwfmPredict a) {
  extern __shared__ uint4 smem[];
  constexpr int Fp = NT * 16, RS = Fp + 4, NTRI = NT * (NT + 1) / 2;
  const int F = a.F, D = a.D, cs = a.cs, C = 1 << cs, PS = a.PS, items = Fp << cs;
  float* Rl = reinterpret_cast<float*>(smem);
  float* rdl = Rl + Fp * RS;
  for (int e = threadIdx.x; e < Fp * RS; e += blockDim.x) {
    const int f = e / RS, g = e - f * RS;
    Rl[e] = f < g && g < F ? a.R[f * F + g] : 0.f;
    if (e < Fp) rdl[e] = e < F ? a.R[e * F + e] : 0.f;
  }
  __syncthreads();
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6, W = blockDim.x >> 6;
  const int i16 = lane & 15, g4 = lane >> 4;
  float* P = rdl + Fp + wv * a.wave_words;
  float* sp = P + Fp * PS;
  int32_t* lslot = reinterpret_cast<int32_t*>(sp + items);
  float* lx = reinterpret_cast<float*>(lslot + 64);
  uint8_t* lpos = reinterpret_cast<uint8_t*>(lx + 64);
  uint8_t* loff = lpos + 64;
  const bool mix32 = a.km.bits <= 32;
  const uint64_t below = (1ull << lane) - 1;
  double loss_acc = 0, corr_acc = 0, cnt = 0;
  for (int64_t b = blockIdx.x * (int64_t)W + wv; b < a.B; b += (int64_t)gridDim.x * W) {
    int64_t lo = a.row_ptr ? a.row_ptr[b] : b * a.width;
    int64_t hi = a.row_ptr ? a.row_ptr[b + 1] : lo + a.width;
    // a corrupted row pointer can never drive a load outside keys[0, nnz)
    lo = lo < 0 ? 0 : (lo > a.nnz ? a.nnz : lo);
    hi = hi < lo ? lo : (hi > a.nnz ? a.nnz : hi);
    const int n = __builtin_amdgcn_readfirstlane((int)(hi - lo));  // nnz < 2^31
    float lin = 0.f;
    int nf = 0;  // lane f: occurrences of field f in the row
    for (int r0 = 0; r0 < n; r0 += 64) {
      // ---- probe phase: lane = occurrence
      const bool ok = r0 + lane < n;
      const int64_t p = ok ? lo + r0 + lane : 0;  // past the row's end: a clamped load
      const uint64_t raw = a.keys[p];
      float x = a.vals ? a.vals[p] : 1.f;
      int f = a.fields ? a.fields[p] : (a.field_of && ok ? a.field_of[r0 + lane] : r0 + lane);
      const uint64_t h = mix32 ? (uint64_t)mix_key32(raw, a.km) : mix_key(raw, a.km);
      const uint64_t idx = home_slot(h, a.mask, a.home_base, a.home_m, a.home_shr) & a.mask;
      const uint4 v = load_slot_head(a.slots, idx);
      const uint64_t hk = head_key(v);
      int32_t slot = hk == h ? (int32_t)idx : -1;  // (cap <= 2^31, checked on the host)
      float w = hk == h ? __uint_as_float(v.z) : 0.f;
      if (ok && hk != h && hk != kEmptyKey) slot = (int32_t)probe_on(a.slots, a.mask, idx, h, w);
      if (!ok) {
        slot = -1;
        w = x = 0.f;
      }
      lin += w * x;
      if (slot < 0 || !in_range(f, F)) f = -1;
      lslot[lane] = slot;
      lx[lane] = x;
      // ---- field lists: counting sort by field (as fwfm_csr_kernel): rank among the earlier
      // lanes of the same field, the count of field fs in lane fs, one scan over the lanes
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
      const int base = __shfl(incl - mine, f < 0 ? 0 : f, 64);  // off[f]
      loff[1 + lane] = (uint8_t)incl;
      if (lane == 0) loff[0] = 0;
      if (f >= 0) lpos[base + rank] = (uint8_t)lane;
      wave_lds_sync();
      // ---- field sums: items (f, c), kGang of a lane at a time
      for (int t0 = 0; t0 < items; t0 += 64 * kGang) {
        float acc[kGang][8], ss[kGang];
        int qi[kGang], qe[kGang], cell[kGang], col[kGang];
        bool any = false;
#pragma unroll
        for (int u = 0; u < kGang; ++u) {
          const int t = t0 + 64 * u + lane;
          const bool on = t < items;
          const int fi = on ? t >> cs : 0, c = on ? t & (C - 1) : 0;
          qi[u] = on ? loff[fi] : 0;
          qe[u] = on ? loff[fi + 1] : 0;
          cell[u] = on ? t : -1;  // sp[t]; P + fi PS + 8 c
          col[u] = 8 * c;
          ss[u] = 0.f;
#pragma unroll
          for (int e = 0; e < 8; ++e) acc[u][e] = 0.f;
          if (r0 > 0 && qi[u] < qe[u]) {  // the sums of the earlier rounds, this lane's own
            const float4* s = reinterpret_cast<const float4*>(P + fi * PS + col[u]);
            const float4 s0 = s[0], s1 = s[1];
            acc[u][0] = s0.x, acc[u][1] = s0.y, acc[u][2] = s0.z, acc[u][3] = s0.w;
            acc[u][4] = s1.x, acc[u][5] = s1.y, acc[u][6] = s1.z, acc[u][7] = s1.w;
            ss[u] = sp[t];
          }
          if (r0 > 0 && qi[u] >= qe[u]) cell[u] = -1;  // nothing to add: the cells stay
          any |= qi[u] < qe[u];
        }
        while (any) {
          uint4 r[kGang];
          float xj[kGang];
          bool ld[kGang];
#pragma unroll
          for (int u = 0; u < kGang; ++u) {
            ld[u] = qi[u] < qe[u];
            const int j = ld[u] ? lpos[qi[u]] & 63 : 0;
            const int32_t sj = lslot[j];
            xj[u] = lx[j];
            ld[u] = ld[u] && sj >= 0;  // (a listed position has a slot)
            r[u] = make_uint4(0, 0, 0, 0);
            // (the address is in range whether or not the load is taken)
            const uint4* src =
                reinterpret_cast<const uint4*>(a.rows + (int64_t)(ld[u] ? sj : 0) * D + col[u]);
            if (ld[u]) r[u] = *src;
          }
          any = false;
#pragma unroll
          for (int u = 0; u < kGang; ++u) {
            if (ld[u]) fwfm_cells_acc(r[u], xj[u], acc[u], ss[u]);
            ++qi[u];
            any |= qi[u] < qe[u];
          }
        }
#pragma unroll
        for (int u = 0; u < kGang; ++u) {
          if (cell[u] < 0) continue;
          float4* s = reinterpret_cast<float4*>(P + (cell[u] >> cs) * PS + col[u]);
          s[0] = make_float4(acc[u][0], acc[u][1], acc[u][2], acc[u][3]);
          s[1] = make_float4(acc[u][4], acc[u][5], acc[u][6], acc[u][7]);
          sp[cell[u]] = ss[u];
        }
      }
      wave_lds_sync();  // the next round rewrites the lists; the pair phase reads all of P
    }
    float part = 0.f;
    if (n > 0) {
      // ---- pair phase: the upper-triangle tiles of P P^T, K = D, then sum Ru o G
      f32x4 g[NTRI];
#pragma unroll
      for (int t = 0; t < NTRI; ++t) g[t] = f32x4{0.f, 0.f, 0.f, 0.f};
      for (int kk = 0; kk < D; kk += 4) {
        float fr[NT];
#pragma unroll
        for (int t = 0; t < NT; ++t) fr[t] = P[(t * 16 + i16) * PS + kk + g4];
        int u = 0;
#pragma unroll
        for (int t1 = 0; t1 < NT; ++t1)
#pragma unroll
          for (int t2 = t1; t2 < NT; ++t2, ++u) g[u] = mfma4(fr[t1], fr[t2], g[u]);
      }
      int u = 0;
#pragma unroll
      for (int t1 = 0; t1 < NT; ++t1)
#pragma unroll
        for (int t2 = t1; t2 < NT; ++t2, ++u)
#pragma unroll
          for (int r = 0; r < 4; ++r)
            part = fmaf(Rl[(t1 * 16 + 4 * g4 + r) * RS + t2 * 16 + i16], g[u][r], part);
      // ---- the diagonal: lane f, by select on n_f >= 2
      if (lane < F && nf >= 2) {
        float sf = 0.f;
        for (int c = 0; c < C; ++c) sf += sp[(lane << cs) + c];
        part = fmaf(rdl[lane], sf, part);
      }
    }
    const float m = wave_allsum(lin + part);
    wave_lds_sync();  // the next row's first round writes the P this one read
    if (lane != 0) continue;
    if (a.margin) a.margin[b] = m;
    if (a.labels) {  // the terms of predict_kernel
      const float y = a.labels[b];
      float loss, coef, coef2;
      loss_terms(m, y, a.loss_type, loss, coef, coef2);
      loss_acc += loss;
      corr_acc += ((y > 0.f) == (m > 0.f)) ? 1.0 : 0.0;
      cnt += 1.0;
      // one count per row, straight into the u64 striped global bins (as ffm_predict.hip: a
      // block histogram in LDS would take 16 KB from the waves' regions)
      if (a.hist)
        atomicAdd(&a.hist[(int64_t)(blockIdx.x % a.hist_stripes) * 2 * a.nbins +
                          auc_bin(m, y, a.nbins)], 1ull);
    }
  }
  if (a.metrics) {  // per-wave DPP sums, lane 63 adds (no barriers)
    const double l = wave_sum_dpp(loss_acc), c = wave_sum_dpp(corr_acc), nn = wave_sum_dpp(cnt);
    if (lane == 63 && nn > 0) {
      double* mt = acc_stripe(a.metrics, a.acc_stripes);
      atomicAdd(&mt[0], l);
      atomicAdd(&mt[1], c);
      atomicAdd(&mt[2], nn);
    }
  }
}

}  // namespace

void fwfm_predict_rows(const TableRef& t, KeyMix km, const void* rows, int D, int F,
                       const float* R, const uint64_t* keys, int64_t nnz, const int64_t* row_ptr,
                       int width, const int32_t* fields, const int32_t* field_of,
                       int64_t field_of_len, const float* vals, const float* labels, int64_t B,
                       int loss_type, float* margin, const StripedAcc& metrics,
                       unsigned long long* hist, int nbins, int hist_stripes, hipStream_t st) {
  auto bad = [](const std::string& s) { throw std::invalid_argument("fwfm_predict_rows: " + s); };
  if (F < 1 || F > 64) bad("1..64 fields, not " + std::to_string(F));
  if (D != 8 && D != 16 && D != 32) bad("D in {8, 16, 32}, not " + std::to_string(D));
  if (!R) bad("no R");
  if (t.cap > (int64_t(1) << 31)) bad("at most 2^31 slots (int32 slot indices)");
  if ((uintptr_t)rows % 16) bad("rows must be 16-byte aligned");
  if (nnz < 0 || nnz >= (int64_t(1) << 31)) bad("0 <= nnz < 2^31");
  if (!row_ptr && width <= 0) bad("needs row_ptr or a fixed width");
  if (row_ptr && nnz > 0 && !fields) bad("rows by row_ptr need a field per occurrence");
  if (!row_ptr && fields) bad("fixed-width rows take a position -> field map, not fields [nnz]");
  if (field_of && (row_ptr || field_of_len != width))
    bad("the position -> field map must have one entry per position of a fixed width");
  if (hist && (nbins <= 0 || hist_stripes < 1)) bad("nbins > 0, at least one stripe");
  if (B <= 0) return;
  const int NT = (F + 15) / 16, Fp = NT * 16, C = D / 8;
  FwfmPredict a = {};
  a.PS = D + 4;
  a.cs = C == 1 ? 0 : (C == 2 ? 1 : 2);
  a.wave_words = Fp * a.PS + Fp * C + kMetaWords;
  // Waves (rows) per block: of the 1..4 that fit 64 KB beside Ru and rd (four always do: at
  // most 17 KB + 4 x 10 KB), the count that puts most waves on a CU, the larger on a tie: the
  // kernel waits on dependent loads. A CU holds what its 160 KB of LDS hold and what the
  // registers allow (the compiler's counts: 4 waves a SIMD up to 48 fields, 3 beyond).
  // F = 39, D = 16: 4,880 B a wave (fwfm_csr's forward form: 7,808 B), 4 waves per block,
  // 4 blocks = 16 waves per CU (by LDS alone: 20).
  const int head = (Fp * (Fp + 4) + Fp) * 4, wave_bytes = a.wave_words * 4;
  const int by_regs = NT == 4 ? 12 : 16;
  int W = 1, per_cu = 0;
  for (int w = 1; w <= 4 && head + w * wave_bytes <= 65536; ++w) {
    const int blocks = std::min(by_regs / w, 163840 / (head + w * wave_bytes));
    if (w * blocks >= W * per_cu) W = w, per_cu = blocks;
  }
  int lg = 0;
  while ((1ll << lg) < t.cap) ++lg;
  a.slots = (const Slot*)t.slots;
  a.mask = (uint64_t)(t.cap - 1);
  a.home_base = t.home_base, a.home_m = t.home_m, a.home_shr = 64 - lg;
  a.km = km;
  a.rows = (const uint16_t*)rows;
  a.R = R;
  a.D = D, a.F = F;
  a.keys = keys, a.nnz = nnz, a.row_ptr = row_ptr, a.width = width;
  a.fields = fields, a.field_of = field_of;
  a.vals = vals, a.labels = labels, a.B = B, a.loss_type = loss_type, a.margin = margin;
  a.metrics = metrics.ptr, a.acc_stripes = metrics.stripes;
  a.hist = hist, a.nbins = nbins, a.hist_stripes = hist_stripes;
  // no more blocks than are resident at once (256 CUs); the waves stride over the rows
  const unsigned g = (unsigned)std::min<int64_t>((B + W - 1) / W, 256 * per_cu);
  const size_t lds = (size_t)head + (size_t)W * wave_bytes;
#define PSAMD_FWFM_PREDICT(N) \
  if (NT == N) fwfm_predict_kernel<N><<<g, 64 * W, lds, st>>>(a)
  PSAMD_FWFM_PREDICT(1);
  PSAMD_FWFM_PREDICT(2);
  PSAMD_FWFM_PREDICT(3);
  PSAMD_FWFM_PREDICT(4);
#undef PSAMD_FWFM_PREDICT
  PSAMD_HIP_CHECK(hipGetLastError());
}

}  // namespace psamd
