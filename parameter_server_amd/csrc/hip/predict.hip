// Scoring a minibatch against a stored model: margins, loss / accuracy sums and a
// bucketed-AUC histogram in ONE launch, straight from the raw keys and the KV table.
//
// Reference: ModelEvaluation (src/app/linear_method/model_evaluation.h:9-74) loads the
// model into a hash map and computes Xw by one lookup per occurrence; a key the model
// does not hold contributes 0. Here the lookup is a read-only probe of the 32-byte slot
// table (kv_slot.cuh): there is no gradient, so nothing is deduplicated, bucketed,
// exchanged or written, and the step's localise -> resolve -> forward chain is not walked.
//
// Row mapping: a lane group of kLPR lanes owns a row and strides over its occurrences,
// kBatch of them per lane and round. A round mixes its raw keys (mix_key, or the 32-bit
// arithmetic of mix_key32 for <= 32 key bits: no separate mix launch, no mixed-key
// buffer), then issues every first-probe load -- one 16-byte load of {key, w, z}, so a
// hit costs one round trip -- before it looks at any of them. Occurrences past the row's
// end load a clamped in-range address and are deselected afterwards (a load inside
// `if (k < e)` would compile to a branch and a full wait per element). Only occurrences
// whose first probe neither hit nor found an empty slot walk on.
//
// The caller synchronises the table before scoring (SparseLRTrainer.flush), so every
// inserted key's weight is published and `w` is read plainly. The kernel never stores
// to the table and has no error word. For given inputs (table bytes included) a margin is
// the same bits on every run: a lane sums its occurrences in index order and the group
// reduces in a fixed xor tree.
#include "predict.h"
#include "kv_slot.cuh"
#include "loss.cuh"
#include <stdexcept>
#include <string>

namespace psamd {

// {key, w, z} of a slot as one 16-byte load (Slot is 32-byte aligned)
__device__ __forceinline__ uint4 load_slot_head(const Slot* __restrict__ slots, uint64_t idx) {
  return *reinterpret_cast<const uint4*>(slots + idx);
}
__device__ __forceinline__ uint64_t head_key(const uint4& v) {
  return ((uint64_t)v.y << 32) | v.x;
}

// The rest of a probe chain whose first slot (idx) held another key. Read-only.
__device__ __forceinline__ float probe_on(const Slot* __restrict__ slots, uint64_t mask,
                                          uint64_t idx, uint64_t h) {
  // TRIP BOUND: at most mask + 1 slots are visited in all (the first probe was slot 0 of
  // the chain), as in resolve_key: on a table without an empty slot an absent key's
  // chain never meets kEmptyKey, and without the bound this loop would not end.
  for (uint64_t probe = 1; probe <= mask; ++probe) {
    idx = (idx + 1) & mask;
    const uint4 v = load_slot_head(slots, idx);
    const uint64_t k = head_key(v);
    if (k == h) return __uint_as_float(v.z);
    if (k == kEmptyKey) return 0.f;
  }
  return 0.f;
}

template <int kLPR, int kBatch, bool kHasRowPtr, bool kMix32>
__global__ void __launch_bounds__(256)
predict_kernel(const Slot* __restrict__ slots, uint64_t mask, uint64_t home_base, uint64_t home_m,
               int home_shr, KeyMix km, const uint64_t* __restrict__ keys, int64_t nnz,
               const int64_t* __restrict__ row_ptr, int width, const float* __restrict__ vals,
               const float* __restrict__ labels, int64_t B, int loss_type,
               float* __restrict__ margin, double* __restrict__ metrics, int acc_stripes,
               unsigned long long* __restrict__ hist, int nbins, int hist_stripes) {
  extern __shared__ uint32_t lhist[];  // [2*nbins] when hist != nullptr
  if (hist) {
    for (int i = threadIdx.x; i < 2 * nbins; i += blockDim.x) lhist[i] = 0;
    __syncthreads();
  }
  const int sub = threadIdx.x % kLPR;
  double loss_acc = 0, corr_acc = 0, cnt = 0;
  const int64_t groups_per_grid = ((int64_t)gridDim.x * blockDim.x) / kLPR;
  const int64_t g0 = ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) / kLPR;
  // (the row loop is rounded up to whole grids of groups: every lane of a wave takes part
  // in the shuffles of every trip)
  for (int64_t r = g0; r < ((B + groups_per_grid - 1) / groups_per_grid) * groups_per_grid;
       r += groups_per_grid) {
    const bool row_ok = r < B;
    int64_t b = 0, e = 0;
    if (row_ok) {
      if (kHasRowPtr) { b = row_ptr[r]; e = row_ptr[r + 1]; }
      else { b = r * width; e = b + width; }
      // a corrupted row pointer can never drive a load outside keys[0, nnz)
      b = b < 0 ? 0 : (b > nnz ? nnz : b);
      e = e < b ? b : (e > nnz ? nnz : e);
    }
    float m = 0.f;
    for (int64_t k0 = b; k0 < e; k0 += kLPR * kBatch) {  // (here e > b: e - 1 is in range)
      uint64_t h[kBatch], idx[kBatch];
      float x[kBatch];
      uint4 v[kBatch];
      bool ok[kBatch];
#pragma unroll
      for (int j = 0; j < kBatch; ++j) {
        const int64_t k = k0 + j * kLPR + sub;
        ok[j] = k < e;
        const int64_t kc = ok[j] ? k : e - 1;
        const uint64_t raw = keys[kc];
        x[j] = vals ? vals[kc] : 1.f;
        h[j] = kMix32 ? (uint64_t)mix_key32(raw, km) : mix_key(raw, km);
      }
#pragma unroll
      for (int j = 0; j < kBatch; ++j) {
        idx[j] = home_slot(h[j], mask, home_base, home_m, home_shr) & mask;
        v[j] = load_slot_head(slots, idx[j]);
      }
#pragma unroll
      for (int j = 0; j < kBatch; ++j) {
        const uint64_t k = head_key(v[j]);
        float w = k == h[j] ? __uint_as_float(v[j].z) : 0.f;
        if (ok[j] && k != h[j] && k != kEmptyKey) w = probe_on(slots, mask, idx[j], h[j]);
        m += ok[j] ? w * x[j] : 0.f;
      }
    }
#pragma unroll
    for (int off = kLPR / 2; off > 0; off >>= 1) m += __shfl_xor(m, off, 64);
    if (!row_ok || sub != 0) continue;
    if (margin) margin[r] = m;
    if (labels) {  // the terms of fwd_row_epilogue (linear.hip)
      const float y = labels[r];
      float loss, coef, coef2;
      loss_terms(m, y, loss_type, loss, coef, coef2);
      loss_acc += loss;
      corr_acc += ((y > 0.f) == (m > 0.f)) ? 1.0 : 0.0;  // evaluation.h:55-57
      cnt += 1.0;
      if (hist) atomicAdd(&lhist[auc_bin(m, y, nbins)], 1u);
    }
  }
  if (metrics) {  // per-wave DPP sums, lane 63 adds (no barriers)
    const double a = wave_sum_dpp(loss_acc), c = wave_sum_dpp(corr_acc), n = wave_sum_dpp(cnt);
    if ((threadIdx.x & 63) == 63 && n > 0) {
      double* mt = acc_stripe(metrics, acc_stripes);
      atomicAdd(&mt[0], a);
      atomicAdd(&mt[1], c);
      atomicAdd(&mt[2], n);
    }
  }
  if (hist) {
    // The bins count a whole validation set, not one minibatch: the block's u32 LDS
    // counts (< 2^32 rows per block and launch) go into u64 global bins, stripe
    // blockIdx % hist_stripes, which a file of any length cannot wrap.
    __syncthreads();
    unsigned long long* hs = hist + (int64_t)(blockIdx.x % hist_stripes) * 2 * nbins;
    for (int i = threadIdx.x; i < 2 * nbins; i += blockDim.x)
      if (lhist[i]) atomicAdd(&hs[i], (unsigned long long)lhist[i]);
  }
}

template <int kLPR, int kBatch>
static void predict_launch(const void* slots, int64_t cap, uint64_t home_base, uint64_t home_m,
                           KeyMix km, const uint64_t* keys, int64_t nnz, const int64_t* row_ptr,
                           int width, const float* vals, const float* labels, int64_t B,
                           int loss_type, float* margin, double* metrics, int acc_stripes,
                           unsigned long long* hist, int nbins, int hist_stripes,
                           hipStream_t st) {
  int lg = 0;
  while ((1ll << lg) < cap) ++lg;
  const size_t lds = hist ? (size_t)2 * nbins * sizeof(uint32_t) : 0;
  // (every block zeroes and scans its 2*nbins LDS histogram: the grid is capped as in
  // linear_fwd, at twice its size, for more probes in flight per CU)
  const int g = grid_for(B * kLPR, 256, 1024);
  const bool rp = row_ptr != nullptr, m32 = km.bits <= 32;
#define PSAMD_PREDICT(RP, M32)                                                                   \
  predict_kernel<kLPR, kBatch, RP, M32><<<g, 256, lds, st>>>(                                    \
      (const Slot*)slots, (uint64_t)(cap - 1), home_base, home_m, 64 - lg, km, keys, nnz,        \
      row_ptr, width, vals, labels, B, loss_type, margin, metrics, acc_stripes, hist, nbins,     \
      hist_stripes)
  if (rp && m32) PSAMD_PREDICT(true, true);
  else if (rp) PSAMD_PREDICT(true, false);
  else if (m32) PSAMD_PREDICT(false, true);
  else PSAMD_PREDICT(false, false);
#undef PSAMD_PREDICT
  PSAMD_HIP_CHECK(hipGetLastError());
}

// lanes per row the host picks for rows of nnz / B occurrences on average: 8 lanes x 5 per
// round cover a 39-wide Criteo row in one round; a whole wave x 2 takes rcv1-like rows
// (~75 occurrences) and longer
static int predict_lanes(int64_t nnz, int64_t B) { return B > 0 && nnz / B >= 64 ? 64 : 8; }

void predict_rows(const TableRef& t, KeyMix km, const uint64_t* keys, int64_t nnz,
                  const int64_t* row_ptr, int width, const float* vals, const float* labels,
                  int64_t B, int loss_type, float* margin, const StripedAcc& metrics,
                  unsigned long long* hist, int nbins, int hist_stripes, int lanes,
                  hipStream_t st) {
  if (B <= 0) return;
  if (lanes == 0) lanes = predict_lanes(nnz, B);
  if (lanes == 64)
    predict_launch<64, 2>(t.slots, t.cap, t.home_base, t.home_m, km, keys, nnz, row_ptr, width,
                          vals, labels, B, loss_type, margin, metrics.ptr, metrics.stripes, hist,
                          nbins, hist_stripes, st);
  else if (lanes == 8)
    predict_launch<8, 5>(t.slots, t.cap, t.home_base, t.home_m, km, keys, nnz, row_ptr, width,
                         vals, labels, B, loss_type, margin, metrics.ptr, metrics.stripes, hist,
                         nbins, hist_stripes, st);
  else
    throw std::invalid_argument("predict_rows: lanes per row must be 0 (auto), 8 or 64");
}

}  // namespace psamd
