// Factorization machine forward + backward (one wavefront per example).
//
// Reference: src/app/factor_machine/ (fm_worker.h, fm.m). The reference FM is an
// unfinished sketch (not in the Makefile); fm.m gives the model it aims at:
//   py = x.w + 1/2 sum_f [ (sum_i x_i v_if)^2 - sum_i x_i^2 v_if^2 ]
//   p  = -y / (1 + exp(y py))              (logistic loss)
//   gv_i = p * (x_i s_f - x_i^2 v_if),  s_f = sum_j x_j v_jf
// (fm.m adds the x^2 v^2 term in the prediction; its gradient uses the standard
// minus sign, which is what is implemented here.)
//
// Inputs are the expanded embedding rows X0 [B*S, D] (bf16, rows of the pulled
// unique keys) and the pulled wide weights; x_i = vals ? vals[i] : 1. Per example:
// lanes own features f = lane, lane + 64 (D <= 128), loop over the S positions to
// build s_f and q_f = sum x^2 v^2; the wide margin is a 64-lane reduction. Outputs:
// coef[b] = p (for the wide-weight gradient), dX0[b*S+i, f] = p (x_i s_f - x_i^2 v_if)
// (bf16, reduced per unique key by emb_grad_reduce), loss / accuracy / AUC histogram.
//
// Three kernels: fm_fwd_bwd_kernel (feature lanes, any D <= 128, expanded X0),
// fm_rows_kernel (lane = position, fixed width S <= 64, D in {8, 16, 32}) and
// fm_csr_kernel (a lane group per row, CSR rows of any width, D in {8, 16, 32}; with
// its forward-only form for scoring).
#include "fm.h"
#include "bf16.cuh"
#include "common.cuh"

#include <algorithm>
#include <stdexcept>

namespace psamd {

__global__ void __launch_bounds__(256)
fm_fwd_bwd_kernel(const uint16_t* __restrict__ X0, const float* __restrict__ vals, int64_t B,
                  int S, int D, const int32_t* __restrict__ local_col,
                  const float* __restrict__ w_local, int64_t w_cap,
                  const float* __restrict__ labels, float* __restrict__ coef_out,
                  uint16_t* __restrict__ dX0, double* __restrict__ metrics,
                  uint32_t* __restrict__ hist, int nbins, int acc_stripes) {
  extern __shared__ uint32_t lhist[];  // [2*nbins]
  for (int i = threadIdx.x; i < 2 * nbins; i += blockDim.x) lhist[i] = 0;
  __syncthreads();
  const int lane = threadIdx.x & 63;
  const int64_t waves = (int64_t)gridDim.x * (blockDim.x / 64);
  double loss_acc = 0, corr_acc = 0, cnt = 0;
  for (int64_t b = blockIdx.x * (int64_t)(blockDim.x / 64) + (threadIdx.x >> 6); b < B;
       b += waves) {
    const int64_t p0 = b * S;
    float s0 = 0.f, s1 = 0.f, q0 = 0.f, q1 = 0.f;
    const int f0 = lane, f1 = lane + 64;
    for (int i = 0; i < S; ++i) {
      const float x = vals ? vals[p0 + i] : 1.f;
      const uint16_t* row = X0 + (p0 + i) * D;
      if (f0 < D) {
        const float v = bf16_to_f32(row[f0]) * x;
        s0 += v;
        q0 += v * v;
      }
      if (f1 < D) {
        const float v = bf16_to_f32(row[f1]) * x;
        s1 += v;
        q1 += v * v;
      }
    }
    float part = 0.5f * (s0 * s0 - q0 + s1 * s1 - q1);
    if (lane < S) {
      const int32_t c = local_col[p0 + lane];
      const float x = vals ? vals[p0 + lane] : 1.f;
      if (in_range(c, w_cap)) part += w_local[c] * x;
    }
    const float m = wave_allsum(part);
    const float y = labels[b] > 0.f ? 1.f : -1.f;
    const float ym = y * m;
    const float tau = 1.f / (1.f + expf(ym));
    const float coef = -y * tau;
    if (lane == 0) {
      coef_out[b] = coef;
      loss_acc += ym > 20.f ? expf(-ym) : (ym < -20.f ? -ym : log1pf(expf(-ym)));
      corr_acc += ((y > 0.f) == (m > 0.f)) ? 1.0 : 0.0;
      cnt += 1.0;
      if (hist) {
        const float pr = 1.f / (1.f + expf(-m));
        const float pb = pr == pr ? fminf(fmaxf(pr * nbins, 0.f), (float)(nbins - 1)) : 0.f;
        atomicAdd(&lhist[(y > 0.f ? nbins : 0) + (int)pb], 1u);
      }
    }
    for (int i = 0; i < S; ++i) {
      const float x = vals ? vals[p0 + i] : 1.f;
      const uint16_t* row = X0 + (p0 + i) * D;
      uint16_t* drow = dX0 + (p0 + i) * D;
      if (f0 < D) drow[f0] = f32_to_bf16(coef * (x * s0 - x * x * bf16_to_f32(row[f0])));
      if (f1 < D) drow[f1] = f32_to_bf16(coef * (x * s1 - x * x * bf16_to_f32(row[f1])));
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
    __syncthreads();
    for (int i = threadIdx.x; i < 2 * nbins; i += blockDim.x)
      if (lhist[i]) atomicAdd(&hist[i], lhist[i]);
  }
}

// Narrow factors (D <= 32, S <= 64): lane = position. Each lane loads its own
// D-wide row with D / 8 16-B loads (the kernel above walks the S positions
// serially with 2-byte loads on D of 64 lanes: latency bound, 94 us at
// B = 16384, S = 39, D = 16), s_f comes from D butterfly sums, and each lane
// writes its own dX0 row with 16-B stores. 4 examples per wave; the AUC
// histogram goes straight to global (one atomic per example, no per-block
// LDS histogram to clear and flush).
//
// Gather mode (X0 == nullptr): the rows are read straight from the embedding store,
// row = rows[idx ? idx[local_col[p]] : local_col[p]], so the [B*S, D] expansion is
// never written and re-read (emb_expand 121 us + its re-read, B = 65536, D = 16).
//
// s_f = sum over the wave of x v_f for all D features: a transpose-reduce butterfly
// (each xor stage hands half of the remaining features to the partner lane, so
// D/2 + D/4 + ... + 1 shuffles, then plain xor sums for the last stages) leaves the
// total of feature f in lane bfly_lane(f); readlane broadcasts it as a wave-uniform
// value. D = 16: 17 shuffles instead of 16 full 6-stage all-sums (96).
template <int D>
__device__ __forceinline__ int bfly_lane(int f) {
  // stage k (offset 32 >> k) decides feature bit (log2(D) - 1 - k)
  int l = 0;
#pragma unroll
  for (int k = 0, n = D; n > 1; ++k, n >>= 1)
    if (f & (n >> 1)) l |= 32 >> k;
  return l;
}

template <int D>
__device__ __forceinline__ void wave_sum_vec(float (&v)[D], float (&s)[D]) {
  const int lane = threadIdx.x & 63;
  float w[D];
#pragma unroll
  for (int j = 0; j < D; ++j) w[j] = v[j];
  int off = 32;
#pragma unroll
  for (int n = D; n > 1; n >>= 1, off >>= 1) {
    const bool hi = lane & off;
#pragma unroll
    for (int j = 0; j < n / 2; ++j) {
      const float keep = hi ? w[j + n / 2] : w[j];
      const float send = hi ? w[j] : w[j + n / 2];
      w[j] = keep + __shfl_xor(send, off, 64);
    }
  }
  float t = w[0];
  for (; off > 0; off >>= 1) t += __shfl_xor(t, off, 64);
  const int ti = __float_as_int(t);
#pragma unroll
  for (int f = 0; f < D; ++f) s[f] = __int_as_float(__builtin_amdgcn_readlane(ti, bfly_lane<D>(f)));
}

template <int D>
__global__ void __launch_bounds__(256)
fm_rows_kernel(const uint16_t* __restrict__ X0, const uint16_t* __restrict__ rows,
               const int64_t* __restrict__ idx, int64_t idx_cap, int64_t rows_cap,
               const float* __restrict__ vals, int64_t B, int S,
               const int32_t* __restrict__ local_col, const float* __restrict__ w_local,
               int64_t w_cap, const float* __restrict__ labels, float* __restrict__ coef_out,
               uint16_t* __restrict__ dX0, double* __restrict__ metrics,
               uint32_t* __restrict__ hist, int nbins, int acc_stripes) {
  const int lane = threadIdx.x & 63;
  const int64_t waves = (int64_t)gridDim.x * (blockDim.x / 64);
  double loss_acc = 0, corr_acc = 0, cnt = 0;
  for (int64_t b = blockIdx.x * (int64_t)(blockDim.x / 64) + (threadIdx.x >> 6); b < B;
       b += waves) {
    const int64_t p = b * S + lane;
    const bool on = lane < S;
    const float x = on ? (vals ? vals[p] : 1.f) : 0.f;
    const int32_t col = on ? local_col[p] : -1;
    const uint16_t* src = nullptr;
    if (X0) {
      if (on) src = X0 + p * D;
    } else if (on) {
      int64_t r = col;
      if (idx) r = in_range(r, idx_cap) ? idx[r] : -1;
      if (in_range(r, rows_cap)) src = rows + r * D;  // unresolved key: zero row
    }
    float v[D];
#pragma unroll
    for (int c = 0; c < D / 8; ++c) {
      uint4 w = make_uint4(0, 0, 0, 0);
      if (src) w = reinterpret_cast<const uint4*>(src)[c];
      const uint16_t* h = reinterpret_cast<const uint16_t*>(&w);
#pragma unroll
      for (int j = 0; j < 8; ++j) v[c * 8 + j] = bf16_to_f32(h[j]);
    }
    float part = 0.f;
    if (on && in_range(col, w_cap)) part = w_local[col] * x;
    float xv[D], s[D], s2 = 0.f;
#pragma unroll
    for (int f = 0; f < D; ++f) {
      xv[f] = x * v[f];
      part -= 0.5f * xv[f] * xv[f];
    }
    wave_sum_vec<D>(xv, s);
#pragma unroll
    for (int f = 0; f < D; ++f) s2 += s[f] * s[f];
    const float m = wave_allsum(part) + 0.5f * s2;
    const float y = labels[b] > 0.f ? 1.f : -1.f;
    const float ym = y * m;
    const float coef = -y / (1.f + expf(ym));
    if (on) {
#pragma unroll
      for (int c = 0; c < D / 8; ++c) {
        uint4 o;
        uint16_t* h = reinterpret_cast<uint16_t*>(&o);
#pragma unroll
        for (int j = 0; j < 8; ++j) {
          const int f = c * 8 + j;
          h[j] = f32_to_bf16(coef * (x * s[f] - x * x * v[f]));
        }
        reinterpret_cast<uint4*>(dX0 + p * D)[c] = o;
      }
    }
    if (lane == 0) {
      coef_out[b] = coef;
      loss_acc += ym > 20.f ? expf(-ym) : (ym < -20.f ? -ym : log1pf(expf(-ym)));
      corr_acc += ((y > 0.f) == (m > 0.f)) ? 1.0 : 0.0;
      cnt += 1.0;
      if (hist) {
        const float pr = 1.f / (1.f + expf(-m));
        const float pb = pr == pr ? fminf(fmaxf(pr * nbins, 0.f), (float)(nbins - 1)) : 0.f;
        atomicAdd(&hist[(y > 0.f ? nbins : 0) + (int)pb], 1u);
      }
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
}

// dE[u, :] += lambda * v_u (L2 on the factors, once per unique key and step, as fm.m);
// v_u = rows[idx ? idx[u] : u] (bf16).
__global__ void fm_l2_kernel(float* __restrict__ dE, const uint16_t* __restrict__ rows,
                             const int64_t* __restrict__ idx, int64_t rows_cap,
                             const int32_t* __restrict__ n_dev, int64_t u_cap, int D,
                             float lambda) {
  const int64_t n = dev_len(n_dev, u_cap) * D;
  for (int64_t e = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; e < n;
       e += (int64_t)gridDim.x * blockDim.x) {
    const int64_t u = e / D;
    const int f = (int)(e - u * D);
    const int64_t r = idx ? idx[u] : u;
    if (in_range(r, rows_cap)) dE[e] += lambda * bf16_to_f32(rows[r * D + f]);
  }
}

// ---------------------------------------------------------------------------------
// fm_csr: rows of any width (CSR minibatches: LIBSVM text, Criteo with missing slots,
// whatever the device feeder produces). "lane = position, one wave = one row" no longer
// fits, so a row is served by a GROUP of L in {16, 32, 64} lanes and a wave holds
// 64 / L rows at a time. Lane g of the group takes positions row_ptr[b] + g, + L, ...:
// the loop bound is the row's own width (0 and 5,000 alike).
//
// Forward: a lane loads each of its rows with D / 8 16-B loads and keeps per-lane
// partial sums over ALL its positions (a_f = sum x v_f: D floats, q = sum_f x^2 v_f^2,
// the wide part x w); only then one transpose-reduce butterfly runs, with xor offsets
// below L only. With T = min(log2 D, log2 L) transposing stages a lane ends with
// max(1, D / L) finished features (L < D: two or four per lane, nothing left to sum);
// L > D finishes its one feature with plain xor sums over the offsets left. s_f is then
// broadcast inside the group with one ds_bpermute per feature (a group is not a wave:
// readlane would hand every row the first group's sums).
//
// Backward: the lane's FIRST position stays in registers between the passes, as the
// packed bf16 words it was loaded as (D / 8 uint4 = D / 2 VGPRs, not D floats: D = 32
// keeps 16 registers and nothing spills) plus x. Those are all positions of a row no
// wider than L, whose factor rows are so read once; positions beyond L are read again
// (from the compact rows_u buffer on one GPU). dX0 rows leave as 16-B stores by the lane
// that owns the position, together with row_of[p] = b for the wide gradient.
//
// Loss, accuracy, AUC bin and coef: once per row by the group's lane 0. kBwd = false is
// the forward-only form: it writes margins[B] and nothing else, keeps nothing.
template <int D, int L>
__device__ __forceinline__ int group_lane(int f) {
  // stage k (offset L >> (k + 1)) decides feature bit (log2(D) - 1 - k)
  int l = 0;
#pragma unroll
  for (int k = 0; (D >> (k + 1)) >= 1 && (L >> (k + 1)) >= 1; ++k)
    if (f & (D >> (k + 1))) l |= L >> (k + 1);
  return l;
}

// s[f] = sum over the lane's group of v[f], for all D features, in every lane of the group
// (wave_sum_vec confined to groups of L lanes)
template <int D, int L>
__device__ __forceinline__ void group_sum_vec(const float (&v)[D], float (&s)[D]) {
  constexpr int N = D > L ? D / L : 1;  // finished features per lane
  const int lane = threadIdx.x & 63;
  float w[D];
#pragma unroll
  for (int j = 0; j < D; ++j) w[j] = v[j];
#pragma unroll
  for (int k = 0; (D >> (k + 1)) >= 1 && (L >> (k + 1)) >= 1; ++k) {
    const int n = D >> k, off = L >> (k + 1);
    const bool hi = lane & off;
#pragma unroll
    for (int j = 0; j < n / 2; ++j) {
      const float keep = hi ? w[j + n / 2] : w[j];
      const float send = hi ? w[j] : w[j + n / 2];
      w[j] = keep + __shfl_xor(send, off, 64);
    }
  }
  if (L > D) {
#pragma unroll
    for (int off = L / D / 2; off > 0; off >>= 1) w[0] += __shfl_xor(w[0], off, 64);
  }
  const int base = lane & ~(L - 1);
#pragma unroll
  for (int f = 0; f < D; ++f) s[f] = __shfl(w[f & (N - 1)], base | group_lane<D, L>(f), 64);
}

template <int D>
struct FmRow {  // one position: its packed bf16 factor row, value and wide weight
  uint4 raw[D / 8];
  float x, w;
};

template <int D>
__device__ __forceinline__ FmRow<D> fm_csr_load(const FmCsr& a, int64_t p) {
  FmRow<D> r;
  r.x = a.vals ? a.vals[p] : 1.f;
  const int64_t col = a.local_col ? (int64_t)a.local_col[p] : p;
  r.w = in_range(col, a.w_cap) ? a.w_local[col] : 0.f;
  int64_t i = col;
  if (a.idx) i = in_range(i, a.idx_cap) ? a.idx[i] : -1;
  const bool ok = in_range(i, a.rows_cap);  // unresolved key: zero row
  const uint4* src = reinterpret_cast<const uint4*>((const uint16_t*)a.rows + (ok ? i : 0) * D);
#pragma unroll
  for (int c = 0; c < D / 8; ++c) r.raw[c] = ok ? src[c] : make_uint4(0, 0, 0, 0);
  return r;
}

// element e of a packed row (bf16 pairs, low half first)
template <int D>
__device__ __forceinline__ float fm_row_at(const FmRow<D>& r, int e) {
  const uint4& q = r.raw[e / 8];
  const uint32_t u = (e / 2) % 4 == 0 ? q.x : (e / 2) % 4 == 1 ? q.y : (e / 2) % 4 == 2 ? q.z : q.w;
  return __uint_as_float(e & 1 ? u & 0xffff0000u : u << 16);
}

template <int D>
__device__ __forceinline__ void fm_csr_acc(const FmRow<D>& r, float (&acc)[D], float& part) {
  part += r.w * r.x;
#pragma unroll
  for (int f = 0; f < D; ++f) {
    const float xv = r.x * fm_row_at<D>(r, f);
    acc[f] += xv;
    part -= 0.5f * xv * xv;
  }
}

template <int D>
__device__ __forceinline__ void fm_csr_store(const FmCsr& a, int64_t p, int32_t b, float coef,
                                             const FmRow<D>& r, const float (&s)[D]) {
  uint4* dst = reinterpret_cast<uint4*>((uint16_t*)a.dX0 + p * D);
#pragma unroll
  for (int c = 0; c < D / 8; ++c) {
    uint32_t o[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const int f = c * 8 + 2 * j;
      const uint32_t lo = f32_to_bf16(coef * (r.x * s[f] - r.x * r.x * fm_row_at<D>(r, f)));
      const uint32_t hi =
          f32_to_bf16(coef * (r.x * s[f + 1] - r.x * r.x * fm_row_at<D>(r, f + 1)));
      o[j] = lo | (hi << 16);
    }
    dst[c] = make_uint4(o[0], o[1], o[2], o[3]);
  }
  a.row_of[p] = b;
}

// (compiled without the packed fp32 forms, v_pk_fma_f32 and its kin: plain fp32 ops only;
// the attribute means something to the device pass alone)
#if defined(__HIP_DEVICE_COMPILE__)
#define PSAMD_FM_CSR_TARGET __attribute__((target("no-packed-fp32-ops")))
#else
#define PSAMD_FM_CSR_TARGET
#endif

template <int D, int L, bool kBwd>
__global__ void PSAMD_FM_CSR_TARGET __launch_bounds__(256) fm_csr_kernel(const FmCsr a) {
  constexpr int kRows = 64 / L;  // rows per wave
  const int lane = threadIdx.x & 63, gl = lane & (L - 1);
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
      lo = lo < 0 ? 0 : (lo > a.nnz ? a.nnz : lo);
      hi = hi < lo ? lo : (hi > a.nnz ? a.nnz : hi);
    }
    float acc[D], part = 0.f;
#pragma unroll
    for (int f = 0; f < D; ++f) acc[f] = 0.f;
    FmRow<D> first;  // the lane's first position (a zero row with x = 0 if it has none)
    first.x = first.w = 0.f;
#pragma unroll
    for (int c = 0; c < D / 8; ++c) first.raw[c] = make_uint4(0, 0, 0, 0);
    if (lo + gl < hi) first = fm_csr_load<D>(a, lo + gl);
    fm_csr_acc<D>(first, acc, part);
    for (int64_t p = lo + gl + L; p < hi; p += L) {
      const FmRow<D> r = fm_csr_load<D>(a, p);
      fm_csr_acc<D>(r, acc, part);
    }
    float s[D], s2 = 0.f;
    group_sum_vec<D, L>(acc, s);
#pragma unroll
    for (int f = 0; f < D; ++f) s2 += s[f] * s[f];
#pragma unroll
    for (int off = L / 2; off > 0; off >>= 1) part += __shfl_xor(part, off, 64);
    const float m = part + 0.5f * s2;
    if (!kBwd) {
      if (live && gl == 0) a.margins[b] = m;
      continue;
    }
    const float y = (live ? a.labels[b] : 1.f) > 0.f ? 1.f : -1.f;
    const float ym = y * m;
    const float coef = -y / (1.f + expf(ym));
    if (lo + gl < hi) fm_csr_store<D>(a, lo + gl, (int32_t)b, coef, first, s);
    for (int64_t p = lo + gl + L; p < hi; p += L) {
      const FmRow<D> r = fm_csr_load<D>(a, p);
      fm_csr_store<D>(a, p, (int32_t)b, coef, r, s);
    }
    if (live && gl == 0) {
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
  }
  if (kBwd && a.metrics) {  // per-wave DPP sums, lane 63 adds (no barriers)
    const double l = wave_sum_dpp(loss_acc), c = wave_sum_dpp(corr_acc), n = wave_sum_dpp(cnt);
    if (lane == 63 && n > 0) {
      double* mt = acc_stripe(a.metrics, a.acc_stripes);
      atomicAdd(&mt[0], l);
      atomicAdd(&mt[1], c);
      atomicAdd(&mt[2], n);
    }
  }
}

// X0 [B*S, D] expanded rows, or X0 == nullptr and rows [rows_cap, D] gathered through
// local_col (and idx [idx_cap] if given); the gather form needs S <= 64, D in {8, 16, 32}.
void fm_fwd_bwd(const void* X0, const void* rows, const int64_t* idx, int64_t idx_cap,
                int64_t rows_cap, const float* vals, int64_t B, int S, int D,
                const int32_t* local_col, const float* w_local, int64_t w_cap, const float* labels,
                float* coef, void* dX0, double* metrics, uint32_t* hist, int nbins,
                int acc_stripes, hipStream_t st) {
  if (S <= 64 && (D == 8 || D == 16 || D == 32)) {
    const unsigned g = (unsigned)std::min<int64_t>((B + 15) / 16, 1 << 20);
#define PSAMD_FM(DD)                                                                          \
  fm_rows_kernel<DD><<<g, 256, 0, st>>>((const uint16_t*)X0, (const uint16_t*)rows, idx, idx_cap, \
                                        rows_cap, vals, B, S, local_col, w_local, w_cap, labels, \
                                        coef, (uint16_t*)dX0, metrics, hist, hist ? nbins : 0,  \
                                        acc_stripes)
    if (D == 8) PSAMD_FM(8);
    else if (D == 16) PSAMD_FM(16);
    else PSAMD_FM(32);
#undef PSAMD_FM
    PSAMD_HIP_CHECK(hipGetLastError());
    return;
  }
  if (!X0) throw std::runtime_error("fm_fwd_bwd: row gather needs S <= 64, D in {8, 16, 32}");
  const int g = grid_for(B * 64, 256, 4096);
  fm_fwd_bwd_kernel<<<g, 256, hist ? 2 * nbins * sizeof(uint32_t) : 0, st>>>(
      (const uint16_t*)X0, vals, B, S, D, local_col, w_local, w_cap, labels, coef,
      (uint16_t*)dX0, metrics, hist, hist ? nbins : 0, acc_stripes);
  PSAMD_HIP_CHECK(hipGetLastError());
}

void fm_l2(float* dE, const void* rows, const int64_t* idx, int64_t rows_cap, const int32_t* n_dev,
           int64_t u_cap, int D, float lambda, hipStream_t st) {
  fm_l2_kernel<<<grid_for(u_cap * D, 256, 4096), 256, 0, st>>>(dE, (const uint16_t*)rows, idx,
                                                               rows_cap, n_dev, u_cap, D, lambda);
  PSAMD_HIP_CHECK(hipGetLastError());
}

// Lanes per row from the mean width: at most 16 -> 16, at most 32 -> 32, else 64, so a
// Criteo row with missing slots (<= 32 wide on average) does not idle half a wave. These
// thresholds are first choices and have NOT been swept on hardware (like predict.hip's
// lane threshold); `lanes` forces a form.
int fm_csr_lanes(int64_t nnz, int64_t B) {
  const int64_t rows = std::max<int64_t>(B, 1);
  return nnz <= 16 * rows ? 16 : (nnz <= 32 * rows ? 32 : 64);
}

namespace {
template <bool kBwd>
void fm_csr_launch(const FmCsr& a, int lanes, hipStream_t st) {
  const int L = lanes ? lanes : fm_csr_lanes(a.nnz, a.B);
  if (a.D != 8 && a.D != 16 && a.D != 32) throw std::runtime_error("fm_csr: D in {8, 16, 32}");
  if (L != 16 && L != 32 && L != 64) throw std::runtime_error("fm_csr: lanes in {16, 32, 64}");
  if (a.B <= 0) return;
  const int64_t per_block = 4 * (64 / L);  // rows a 256-thread block holds at a time
  const unsigned g = (unsigned)std::min<int64_t>((a.B + per_block - 1) / per_block, 1 << 20);
#define PSAMD_FM_CSR(DD, LL) \
  if (a.D == DD && L == LL) fm_csr_kernel<DD, LL, kBwd><<<g, 256, 0, st>>>(a)
  PSAMD_FM_CSR(8, 16);
  PSAMD_FM_CSR(8, 32);
  PSAMD_FM_CSR(8, 64);
  PSAMD_FM_CSR(16, 16);
  PSAMD_FM_CSR(16, 32);
  PSAMD_FM_CSR(16, 64);
  PSAMD_FM_CSR(32, 16);
  PSAMD_FM_CSR(32, 32);
  PSAMD_FM_CSR(32, 64);
#undef PSAMD_FM_CSR
  PSAMD_HIP_CHECK(hipGetLastError());
}
}  // namespace

void fm_csr(const FmCsr& a, int lanes, hipStream_t st) { fm_csr_launch<true>(a, lanes, st); }
void fm_csr_margins(const FmCsr& a, int lanes, hipStream_t st) {
  fm_csr_launch<false>(a, lanes, st);
}

}  // namespace psamd
