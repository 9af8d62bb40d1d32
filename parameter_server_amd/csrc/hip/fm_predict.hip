// Scoring a minibatch against a stored factorization machine: margins, loss / accuracy
// sums and the bucketed-AUC histogram in ONE launch, straight from the raw keys, the KV
// table and the bf16 factor rows at the slot index of every key (EmbeddingShard.rows).
//
//   margin = sum_i x_i w_i + 1/2 sum_f [ (sum_i x_i v_if)^2 - sum_i x_i^2 v_if^2 ]   (fm.m)
//
// The composed route (mix in torch, table.resolve(insert=False), torch.where, fm_csr's
// forward-only form) writes a slot and a weight per occurrence to HBM and reads them back,
// and fm_csr keeps all D partial sums of a position in one lane, which ends at D = 32.
// Here a group of L lanes (16, 32 or 64; 64 / L rows per wave) owns a row and runs two
// phases per round of L occurrences, and nothing per occurrence leaves the registers.
//
// Probe phase, lane = occurrence (the probe of predict.hip, through probe.cuh): mix the raw
// key, one 16-byte {key, w, z} first-probe load per lane at a clamped address, all of them
// issued before any is inspected; only a miss on an occupied slot walks its chain. Result
// per lane: the slot index (int32, -1: absent or past the row's end), w and x. An absent
// key is a zero row with a zero weight, as in FMTrainer.predict.
//
// Factor phase, a position's row split across lanes BY D: with C = the power of two
// >= D / 8 (1 .. 16), C neighbouring lanes serve one position and lane slice c = gl % C
// loads the 16 bytes at rows + slot * D + 8 c, so a position's row is one contiguous
// 2 D-byte read of C lanes and D = 24, 40, ... simply leave the slices with 8 c >= D idle.
// A sub-round covers L / C positions, a round C sub-rounds; slot and x of a position reach
// its C lanes by a shuffle from the lane that probed it (group base lane | position: a
// group is not a wave). The loads of up to 4 sub-rounds are in flight together, and a
// sub-round in which no group of the wave has a present key is skipped wave-uniformly (the
// ballot of slot >= 0 against the sub-round's probe lanes). Every lane keeps 8 partial sums
// a[e] (features 8 c + e), q = sum (x v)^2 and the linear part: the register cost does not
// depend on D.
//
// After the row: a[] is summed over the lanes of equal slice (xor offsets C .. L / 2), so
// every lane holds s_f of its 8 features; t = sum_e a[e]^2 is summed over the slices (xor
// offsets below C), the linear part and q over the whole group. margin = lin + (t - q) / 2
// with no transpose and no broadcast of s_f. Lane 0 of the group writes it and, with
// labels, the loss terms, the f64 sums (per-wave DPP) and the block's u32 LDS histogram,
// flushed into the u64 striped global bins as predict_kernel does.
//
// Every sum has a fixed order that depends on the row's occurrences alone (never on the
// slot a key sits in): a margin is the same bits on every run and for every layout of the
// same model. Read-only on the table and the rows; no error word.
#include "fm_predict.h"
#include "fm.h"
#include "loss.cuh"
#include "probe.cuh"

#include <algorithm>
#include <stdexcept>
#include <string>

namespace psamd {

namespace {

struct FmPredict {
  const Slot* slots;
  uint64_t mask, home_base, home_m;
  int home_shr;
  KeyMix km;
  const uint16_t* rows;  // [mask + 1, D] bf16
  int D;
  const uint64_t* keys;
  int64_t nnz;
  const int64_t* row_ptr;
  int width;
  const float* vals;
  const float* labels;
  int64_t B;
  int loss_type;
  float* margin;
  double* metrics;
  int acc_stripes;
  unsigned long long* hist;
  int nbins, hist_stripes;
};

// 8 bf16 features of one position times its value: a[e] += x v_e, q += sum_e (x v_e)^2
// (the squares of a position are summed first, so q grows by one addition per position)
__device__ __forceinline__ void fm_slice_acc(const uint4& r, float x, float (&a)[8], float& q) {
  const uint32_t u[4] = {r.x, r.y, r.z, r.w};
  float p = 0.f;
#pragma unroll
  for (int j = 0; j < 4; ++j) {  // bf16 pairs, low half first
    const float lo = x * __uint_as_float(u[j] << 16);
    const float hi = x * __uint_as_float(u[j] & 0xffff0000u);
    a[2 * j] += lo;
    a[2 * j + 1] += hi;
    p += lo * lo;
    p += hi * hi;
  }
  q += p;
}

// (_build.py compiles this unit without the packed fp32 forms, v_pk_fma_f32 and its kin, as
// a target feature of the whole unit: a per-kernel target attribute would keep every header
// function, __shfl included, from being inlined)
template <int C, int L>
__global__ void __launch_bounds__(256)
fm_predict_kernel(const FmPredict a) {
  static_assert(C >= 1 && C <= 16 && L >= C && L <= 64, "C lanes per position, L per row");
  constexpr int kRows = 64 / L;          // rows per wave
  constexpr int P = L / C;               // positions per sub-round
  constexpr int kGang = C < 4 ? C : 4;   // sub-rounds whose loads are in flight together
  // the lanes that probed the positions of sub-round 0, in every group of the wave
  constexpr uint64_t kRep = L == 64 ? 1ull : (L == 32 ? 0x0000000100000001ull
                                                      : 0x0001000100010001ull);
  constexpr uint64_t kSub0 = P == 64 ? ~0ull : ((1ull << P) - 1) * kRep;
  extern __shared__ uint32_t lhist[];  // [2*nbins] when hist != nullptr
  if (a.hist) {
    for (int i = threadIdx.x; i < 2 * a.nbins; i += blockDim.x) lhist[i] = 0;
    __syncthreads();
  }
  const int lane = threadIdx.x & 63, gl = lane & (L - 1);
  const int c8 = (gl % C) * 8;         // first feature of this lane's slice
  const bool slice_on = c8 < a.D;      // D = 24, 40, ...: the last slices hold nothing
  const int src0 = (lane - gl) + gl / C;  // the lane that probed this lane's position
  const uint16_t* rows_c = a.rows + (slice_on ? c8 : 0);
  const bool mix32 = a.km.bits <= 32;
  const int64_t stride = (int64_t)gridDim.x * (blockDim.x / 64) * kRows;
  double loss_acc = 0, corr_acc = 0, cnt = 0;
  // b0 is wave-uniform: every lane stays in the loop for the shuffles, rows past B are
  // rows of width 0
  for (int64_t b0 = (blockIdx.x * (int64_t)(blockDim.x / 64) + (threadIdx.x >> 6)) * kRows;
       b0 < a.B; b0 += stride) {
    const int64_t b = b0 + lane / L;
    const bool live = b < a.B;
    int64_t lo = 0, hi = 0;
    if (live) {
      lo = a.row_ptr ? a.row_ptr[b] : b * a.width;
      hi = a.row_ptr ? a.row_ptr[b + 1] : lo + a.width;
      // a corrupted row pointer can never drive a load outside keys[0, nnz)
      lo = lo < 0 ? 0 : (lo > a.nnz ? a.nnz : lo);
      hi = hi < lo ? lo : (hi > a.nnz ? a.nnz : hi);
    }
    float acc[8], q = 0.f, lin = 0.f;
#pragma unroll
    for (int e = 0; e < 8; ++e) acc[e] = 0.f;
    // a round per L occurrences, as many as the widest row of the wave needs (some group
    // has k0 < hi: nnz > 0 and keys[0] exists)
    for (int64_t k0 = lo; __ballot(k0 < hi) != 0; k0 += L) {
      // ---- probe phase: lane = occurrence
      const int64_t k = k0 + gl;
      const bool ok = k < hi;
      const int64_t kc = ok ? k : 0;  // past the row's end: a clamped load, deselected below
      const uint64_t raw = a.keys[kc];
      float x = a.vals ? a.vals[kc] : 1.f;
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
      // ---- factor phase: C lanes per position, L / C positions per sub-round
      const uint64_t present = __ballot(slot >= 0);
#pragma unroll
      for (int j0 = 0; j0 < C; j0 += kGang) {
        uint4 r[kGang];
        float xp[kGang];
#pragma unroll
        for (int j = 0; j < kGang; ++j) {
          r[j] = make_uint4(0, 0, 0, 0);
          xp[j] = 0.f;
          if (!(present & (kSub0 << ((j0 + j) * P)))) continue;  // wave-uniform
          const int src = src0 + (j0 + j) * P;
          const int32_t sp = __shfl(slot, src, 64);
          xp[j] = __shfl(x, src, 64);
          const bool on = sp >= 0 && slice_on;
          // (the address is in range whether or not the load is taken)
          const uint4* p = reinterpret_cast<const uint4*>(rows_c + (int64_t)(on ? sp : 0) * a.D);
          if (on) r[j] = *p;
        }
#pragma unroll
        for (int j = 0; j < kGang; ++j) {
          if (!(present & (kSub0 << ((j0 + j) * P)))) continue;
          fm_slice_acc(r[j], xp[j], acc, q);
        }
      }
    }
    // s_f of this lane's 8 features: over the lanes of equal slice
#pragma unroll
    for (int off = C; off < L; off <<= 1) {
#pragma unroll
      for (int e = 0; e < 8; ++e) acc[e] += __shfl_xor(acc[e], off, 64);
    }
    float t = 0.f;
#pragma unroll
    for (int e = 0; e < 8; ++e) t += acc[e] * acc[e];
#pragma unroll
    for (int off = 1; off < C; off <<= 1) t += __shfl_xor(t, off, 64);  // over the slices
#pragma unroll
    for (int off = 1; off < L; off <<= 1) {
      lin += __shfl_xor(lin, off, 64);
      q += __shfl_xor(q, off, 64);
    }
    const float m = lin + 0.5f * (t - q);
    if (!live || gl != 0) continue;
    if (a.margin) a.margin[b] = m;
    if (a.labels) {  // the terms of predict_kernel
      const float y = a.labels[b];
      float loss, coef, coef2;
      loss_terms(m, y, a.loss_type, loss, coef, coef2);
      loss_acc += loss;
      corr_acc += ((y > 0.f) == (m > 0.f)) ? 1.0 : 0.0;
      cnt += 1.0;
      if (a.hist) atomicAdd(&lhist[auc_bin(m, y, a.nbins)], 1u);
    }
  }
  if (a.metrics) {  // per-wave DPP sums, lane 63 adds (no barriers)
    const double l = wave_sum_dpp(loss_acc), c = wave_sum_dpp(corr_acc), n = wave_sum_dpp(cnt);
    if (lane == 63 && n > 0) {
      double* mt = acc_stripe(a.metrics, a.acc_stripes);
      atomicAdd(&mt[0], l);
      atomicAdd(&mt[1], c);
      atomicAdd(&mt[2], n);
    }
  }
  if (a.hist) {
    // the block's u32 LDS counts go into u64 global bins, stripe blockIdx % hist_stripes,
    // which a file of any length cannot wrap (predict.hip)
    __syncthreads();
    unsigned long long* hs = a.hist + (int64_t)(blockIdx.x % a.hist_stripes) * 2 * a.nbins;
    for (int i = threadIdx.x; i < 2 * a.nbins; i += blockDim.x)
      if (lhist[i]) atomicAdd(&hs[i], (unsigned long long)lhist[i]);
  }
}

template <int C>
void fm_predict_launch(const FmPredict& a, int L, hipStream_t st) {
  const size_t lds = a.hist ? (size_t)2 * a.nbins * sizeof(uint32_t) : 0;
  // a 256-thread block holds 4 * 64 / L rows at a time; every block zeroes and scans its
  // LDS histogram, so the grid is capped at 8 blocks per CU (256 CUs). The cap has NOT
  // been swept on hardware.
  const int64_t per_block = 4 * (64 / L);
  const unsigned g = (unsigned)std::min<int64_t>((a.B + per_block - 1) / per_block, 2048);
  if (L == 16) fm_predict_kernel<C, 16><<<g, 256, lds, st>>>(a);
  else if (L == 32) fm_predict_kernel<C, 32><<<g, 256, lds, st>>>(a);
  else fm_predict_kernel<C, 64><<<g, 256, lds, st>>>(a);
  PSAMD_HIP_CHECK(hipGetLastError());
}

}  // namespace

void fm_predict_rows(const TableRef& t, KeyMix km, const void* rows, int D, const uint64_t* keys,
                     int64_t nnz, const int64_t* row_ptr, int width, const float* vals,
                     const float* labels, int64_t B, int loss_type, float* margin,
                     const StripedAcc& metrics, unsigned long long* hist, int nbins,
                     int hist_stripes, int lanes, hipStream_t st) {
  if (D <= 0 || D % 8 || D > 128)
    throw std::invalid_argument("fm_predict_rows: D must be a multiple of 8 up to 128");
  if (t.cap > (int64_t(1) << 31))
    throw std::invalid_argument("fm_predict_rows: at most 2^31 slots (int32 slot indices)");
  if ((uintptr_t)rows % 16)
    throw std::invalid_argument("fm_predict_rows: rows must be 16-byte aligned");
  const int L = lanes ? lanes : fm_csr_lanes(nnz, B);
  if (L != 16 && L != 32 && L != 64)
    throw std::invalid_argument("fm_predict_rows: lanes per row must be 0 (auto), 16, 32 or 64");
  if (B <= 0) return;
  int lg = 0;
  while ((1ll << lg) < t.cap) ++lg;
  const FmPredict a = {(const Slot*)t.slots, (uint64_t)(t.cap - 1), t.home_base, t.home_m,
                       64 - lg, km, (const uint16_t*)rows, D, keys, nnz, row_ptr, width, vals,
                       labels, B, loss_type, margin, metrics.ptr, metrics.stripes, hist, nbins,
                       hist_stripes};
  // C lanes per position: the power of two >= D / 8
  if (D <= 8) fm_predict_launch<1>(a, L, st);
  else if (D <= 16) fm_predict_launch<2>(a, L, st);
  else if (D <= 32) fm_predict_launch<4>(a, L, st);
  else if (D <= 64) fm_predict_launch<8>(a, L, st);
  else fm_predict_launch<16>(a, L, st);
}

}  // namespace psamd
