// Scoring a minibatch against a stored field-aware factorization machine: margins, loss /
// accuracy sums and the bucketed-AUC histogram in ONE launch, straight from the raw keys, the
// KV table and the bf16 factor rows at the slot index of every key (EmbeddingShard.rows),
// for rows of any width.
//
//   margin = sum_i x_i w_i + sum_{i<j} x_i x_j <v_{i,f_j}, v_{j,f_i}>,  v_{i,f} = row_i[f k, +k)
//
// With A[f][g] = sum over the positions i of field f of x_i v_{i,g} (so A[f] is the
// x-weighted sum of the whole rows of field f's positions, Dr floats),
//
//   sum_{i<j} ... = sum_{f<g} <A[f][g], A[g][f]> + 1/2 (sum_f |A[f][f]|^2 - sum_i x_i^2 |v_{i,f_i}|^2)
//
// the FM's "square of sums minus sum of squares" per field pair: O(n Dr + F^2 k) per row
// where the training tile (ffm.hip, ffm_csr.hip) pays O(n^2 k), every factor row is read
// from HBM once, and nothing has to fit a tile. The rules are ffm_csr's: a field outside
// [0, F) keeps its linear term and enters no pair, an absent key contributes nothing, a key
// that occurs twice is two positions, same-field pairs count.
//
// One wavefront per row, grid-stride over B, on a per-wave LDS region
//   A f32 [F][S = Dr + 4] | slot int32 [64] | x f32 [64] | pos bytes [64] | off bytes [F + 1]
// (S / 4 is odd: the pair phase's reads of A[g][f k, +k) for neighbouring g start 4 S bytes
// apart and spread over the banks, and every row of A stays 16-byte aligned). A row runs in
// rounds of 64 occurrences:
//
// Probe phase, lane = occurrence (fm_predict.hip's probe, through probe.cuh): mix the raw
//   key, one 16-byte first-probe load per lane at a clamped address, all issued before any is
//   inspected; only a miss on an occupied slot walks its chain. lin += w x in the lane. The
//   slot and x go to LDS; a lane without a slot or with a field outside [0, F) is in no list.
// Field lists (ffm_csr_kernel's stable counting sort, in registers and cross-lane moves):
//   pos[] holds the round's listed positions by field, in position order, off[f] the start.
// Accumulate phase, items (f, c) = field x 16-byte chunk of the row, item t = f C + c on
//   lane t % 64, the same dealing in every round: the lane walks field f's list and for every
//   position j loads rows[slot_j][8 c, +8) from global memory and adds x_j v into its 8 cells
//   A[f][8 c, +8). A lane takes 4 items at a time, so up to 4 loads are in flight per lane; the
//   cells sit in registers during the walk (read back from LDS in a later round, zero in the
//   first) and are written once. One writer per cell, ascending position order over the
//   whole row. The item whose chunk holds columns [f k, f k + k) also sums the diagonal
//   q += x_j^2 |v_{j,f}|^2.
// Pair phase (after the last round): the pairs f <= g, pair t on lane t % 64 in row-major
//   order of the upper triangle, k FMAs each, f == g halved.
//   m = wave_allsum(lin + pairs - q / 2).
// Epilogue: fm_predict_kernel's (lane 0: margin, loss terms, f64 sums by per-wave DPP), but
//   the AUC count of a row is one atomic add into the u64 striped global bins: a block's LDS
//   histogram would cost 16 KB of the LDS that bounds this kernel's occupancy.
//
// Every sum has an order fixed by the row's occurrences and (F, k, Dr) alone, never by the
// slot a key sits in: a margin is the same bits on every run, for every table layout, and
// for a fixed-width row and the same row in CSR form. Read-only on the table and the rows;
// a slot index is used for a load only after the probe has produced it.
#include "ffm_predict.h"
#include "ffm_tile.cuh"
#include "loss.cuh"
#include "probe.cuh"

#include <algorithm>
#include <stdexcept>
#include <string>

namespace psamd {

namespace {

constexpr int kMetaWords = 64 + 64 + 16 + 20;  // slot, x, pos bytes, off bytes (F + 1 <= 80)
constexpr int kGang = 4;                       // items of a lane whose loads fly together

struct FfmPredict {
  const Slot* slots;
  uint64_t mask, home_base, home_m;
  int home_shr;
  KeyMix km;
  const uint16_t* rows;  // [mask + 1, Dr] bf16
  int Dr, F, C, S;       // C = Dr / 8 chunks, S = A's row stride in floats
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

// k floats of A at a k-float boundary
template <int K>
__device__ __forceinline__ void lds_vec(const float* p, float (&v)[K]) {
  if constexpr (K == 2) {
    const float2 t = *reinterpret_cast<const float2*>(p);
    v[0] = t.x, v[1] = t.y;
  } else {
#pragma unroll
    for (int h = 0; h < K / 4; ++h) {
      const float4 t = reinterpret_cast<const float4*>(p)[h];
      v[4 * h] = t.x, v[4 * h + 1] = t.y, v[4 * h + 2] = t.z, v[4 * h + 3] = t.w;
    }
  }
}

// cells += x v for the 8 bf16 of one chunk; with d >= 0 (the chunk holds the position's own
// field at columns [d, d + K)) also q += sum (x v_e)^2 over them
template <int K>
__device__ __forceinline__ void ffm_cells_acc(const uint4& r, float x, int d, float (&a)[8],
                                              float& q) {
  const uint32_t u[4] = {r.x, r.y, r.z, r.w};
  float p = 0.f;
#pragma unroll
  for (int j = 0; j < 4; ++j) {  // bf16 pairs, low half first
    const float lo = x * __uint_as_float(u[j] << 16);
    const float hi = x * __uint_as_float(u[j] & 0xffff0000u);
    a[2 * j] += lo;
    a[2 * j + 1] += hi;
    if (2 * j >= d && 2 * j < d + K) {  // (d and K are even: a pair is in or out as a whole)
      p += lo * lo;
      p += hi * hi;
    }
  }
  if (d >= 0) q += p;
}

template <int K>
__global__ void __launch_bounds__(256) ffm_predict_kernel(const FfmPredict a) {
  extern __shared__ uint4 smem[];
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6, W = blockDim.x >> 6;
  float* A = reinterpret_cast<float*>(smem) + wv * a.wave_words;
  int32_t* lslot = reinterpret_cast<int32_t*>(A + a.F * a.S);
  float* lx = reinterpret_cast<float*>(lslot + 64);
  uint8_t* lpos = reinterpret_cast<uint8_t*>(lx + 64);
  uint8_t* loff = lpos + 64;
  const int F = a.F, C = a.C, S = a.S, items = F * C;
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
    float lin = 0.f, q = 0.f;
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
      // ---- field lists: counting sort by field (as ffm_csr_kernel): rank among the earlier
      // lanes of the same field, the count of field fs in lane fs, one scan over the lanes
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
      loff[1 + lane] = (uint8_t)incl;
      if (lane == 0) loff[0] = 0;
      if (f >= 0) lpos[base + rank] = (uint8_t)lane;
      wave_lds_sync();
      // ---- accumulate phase: items (f, c), kGang of a lane at a time
      for (int t0 = 0; t0 < items; t0 += 64 * kGang) {
        float acc[kGang][8];
        int qi[kGang], qe[kGang], cell[kGang], col[kGang], dg[kGang];
        bool any = false;
#pragma unroll
        for (int u = 0; u < kGang; ++u) {
          const int t = t0 + 64 * u + lane;
          const bool on = t < items;
          const int fi = on ? t / C : 0, c = on ? t - fi * C : 0;
          qi[u] = on ? loff[fi] : 0;
          qe[u] = on ? loff[fi + 1] : 0;
          cell[u] = on ? fi * S + 8 * c : -1;
          col[u] = 8 * c;
          dg[u] = (fi * K) >> 3 == c ? (fi * K) & 7 : -1;
#pragma unroll
          for (int e = 0; e < 8; ++e) acc[u][e] = 0.f;
          if (r0 > 0 && qi[u] < qe[u]) {  // the sums of the earlier rounds, this lane's own
            const float4* s = reinterpret_cast<const float4*>(A + cell[u]);
            const float4 s0 = s[0], s1 = s[1];
            acc[u][0] = s0.x, acc[u][1] = s0.y, acc[u][2] = s0.z, acc[u][3] = s0.w;
            acc[u][4] = s1.x, acc[u][5] = s1.y, acc[u][6] = s1.z, acc[u][7] = s1.w;
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
                reinterpret_cast<const uint4*>(a.rows + (int64_t)(ld[u] ? sj : 0) * a.Dr + col[u]);
            if (ld[u]) r[u] = *src;
          }
          any = false;
#pragma unroll
          for (int u = 0; u < kGang; ++u) {
            if (ld[u]) ffm_cells_acc<K>(r[u], xj[u], dg[u], acc[u], q);
            ++qi[u];
            any |= qi[u] < qe[u];
          }
        }
#pragma unroll
        for (int u = 0; u < kGang; ++u) {
          if (cell[u] < 0) continue;
          float4* s = reinterpret_cast<float4*>(A + cell[u]);
          s[0] = make_float4(acc[u][0], acc[u][1], acc[u][2], acc[u][3]);
          s[1] = make_float4(acc[u][4], acc[u][5], acc[u][6], acc[u][7]);
        }
      }
      wave_lds_sync();  // the next round rewrites the lists; the pair phase reads all of A
    }
    // ---- pair phase: the upper triangle f <= g in row-major order, pair t on lane t % 64
    float part = 0.f;
    if (n > 0) {
      int f = 0, g = lane;
      while (g >= F && f < F) ++f, g += f - F;
      while (f < F) {
        float u[K], v[K];
        lds_vec<K>(A + f * S + g * K, u);
        lds_vec<K>(A + g * S + f * K, v);
        float d = 0.f;
#pragma unroll
        for (int e = 0; e < K; ++e) d = fmaf(u[e], v[e], d);
        part += f == g ? 0.5f * d : d;
        g += 64;
        while (g >= F && f < F) ++f, g += f - F;
      }
    }
    const float m = wave_allsum(lin + part - 0.5f * q);
    wave_lds_sync();  // the next row's first round writes the A this one read
    if (lane != 0) continue;
    if (a.margin) a.margin[b] = m;
    if (a.labels) {  // the terms of predict_kernel
      const float y = a.labels[b];
      float loss, coef, coef2;
      loss_terms(m, y, a.loss_type, loss, coef, coef2);
      loss_acc += loss;
      corr_acc += ((y > 0.f) == (m > 0.f)) ? 1.0 : 0.0;
      cnt += 1.0;
      // one count per row, straight into the u64 striped global bins: a block histogram in
      // LDS (fm_predict.hip) would take 16 KB from the field sums and halve the waves per CU
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

void ffm_predict_rows(const TableRef& t, KeyMix km, const void* rows, int Dr, int F, int k,
                      const uint64_t* keys, int64_t nnz, const int64_t* row_ptr, int width,
                      const int32_t* fields, const int32_t* field_of, int64_t field_of_len,
                      const float* vals, const float* labels, int64_t B, int loss_type,
                      float* margin, const StripedAcc& metrics, unsigned long long* hist,
                      int nbins, int hist_stripes, hipStream_t st) {
  auto bad = [](const std::string& s) { throw std::invalid_argument("ffm_predict_rows: " + s); };
  if (k != 2 && k != 4 && k != 8) bad("k in {2, 4, 8}, not " + std::to_string(k));
  if (Dr <= 0 || Dr % 8 || Dr > 128 || F < 1 || F * k > Dr)
    bad("rows of F * k <= Dr <= 128 columns, Dr % 8 == 0 (F = " + std::to_string(F) +
        ", k = " + std::to_string(k) + ", Dr = " + std::to_string(Dr) + ")");
  if (t.cap > (int64_t(1) << 31)) bad("at most 2^31 slots (int32 slot indices)");
  if ((uintptr_t)rows % 16) bad("rows must be 16-byte aligned");
  if (nnz < 0 || nnz >= (int64_t(1) << 31)) bad("0 <= nnz < 2^31");
  if (!row_ptr && width <= 0) bad("needs row_ptr or a fixed width");
  if (row_ptr && nnz > 0 && !fields) bad("rows by row_ptr need a field per occurrence");
  if (!row_ptr && fields) bad("fixed-width rows take a position -> field map, not fields [nnz]");
  if (field_of && (row_ptr || field_of_len != width))
    bad("the position -> field map must have one entry per position of a fixed width");
  if (hist && nbins <= 0) bad("nbins > 0");
  FfmPredict a = {};
  a.S = Dr + 4;
  a.wave_words = F * a.S + kMetaWords;
  if (B <= 0) return;
  // Waves (rows) per block: of the 1..4 that fit 64 KB (one always does: at most 33 KB), the
  // count that puts most waves on a CU's 160 KB of LDS, the larger on a tie: the kernel waits
  // on dependent loads, and LDS, not registers, bounds its occupancy. F = 39, k = 2: 1 wave
  // per block, 11 per CU (4 per block: 8 per CU).
  int W = 1, per_cu = 0;
  for (int w = 1; w <= 4 && w * a.wave_words <= 65536 / 4; ++w) {
    const int blocks = std::min(32, 163840 / 4 / (w * a.wave_words));
    if (w * blocks >= W * per_cu) W = w, per_cu = blocks;
  }
  int lg = 0;
  while ((1ll << lg) < t.cap) ++lg;
  a.slots = (const Slot*)t.slots;
  a.mask = (uint64_t)(t.cap - 1);
  a.home_base = t.home_base, a.home_m = t.home_m, a.home_shr = 64 - lg;
  a.km = km;
  a.rows = (const uint16_t*)rows;
  a.Dr = Dr, a.F = F, a.C = Dr / 8;
  a.keys = keys, a.nnz = nnz, a.row_ptr = row_ptr, a.width = width;
  a.fields = fields, a.field_of = field_of;
  a.vals = vals, a.labels = labels, a.B = B, a.loss_type = loss_type, a.margin = margin;
  a.metrics = metrics.ptr, a.acc_stripes = metrics.stripes;
  a.hist = hist, a.nbins = nbins, a.hist_stripes = hist_stripes;
  // no more blocks than are resident at once (256 CUs); the waves stride over the rows
  const unsigned g = (unsigned)std::min<int64_t>((B + W - 1) / W, 256 * per_cu);
  const size_t lds = (size_t)W * a.wave_words * 4;
  if (k == 2) ffm_predict_kernel<2><<<g, 64 * W, lds, st>>>(a);
  else if (k == 4) ffm_predict_kernel<4><<<g, 64 * W, lds, st>>>(a);
  else ffm_predict_kernel<8><<<g, 64 * W, lds, st>>>(a);
  PSAMD_HIP_CHECK(hipGetLastError());
}

}  // namespace psamd
