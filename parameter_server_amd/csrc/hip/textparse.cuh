// What the device text parsers (textparse.hip, pstext.hip, adtext.hip) share: the work
// decomposition (16 KiB of text per 1024-thread workgroup), the header words, the
// associative carries and the workgroup scan over them, the clamped load of a span into LDS,
// the header / capacity step that closes a scan launch, the bytes an emit thread reads a
// token from, the reduction that closes an emit launch, and the finish launches (row-width
// range with the optional LIBSVM order check, keys mod hash_mod). Each parser adds its own
// classify, count, scan and emit kernels (they know the grammar). The host side of the
// finish launches (tp_fgrid, tp_finish) is here as well. Included by .hip files only;
// everything has internal linkage.
#pragma once
#include "common.cuh"
#include "textparse.h"
#include "../core/textnum.h"

#include <cstdint>

namespace psamd {

namespace {

constexpr int kTpBlk = 1024;                // threads per workgroup
constexpr int kTpBytes = 16;                // text bytes per thread
constexpr int kTpSpan = kTpBlk * kTpBytes;  // 16 KiB of text per workgroup
constexpr int kTpWaves = kTpBlk / kWave;

// header words (int32)
enum { H_ROWS, H_NNZ, H_MINW, H_MAXW, H_NONUNIT, H_BAD, H_DEFER, H_CAP, H_WORDS };

// "line holds a token" carry as a function of the carry-in: a | (b & in), packed a | b<<1.
struct LineFn {
  static constexpr uint32_t ident = 2;
  __device__ static uint32_t op(uint32_t l, uint32_t r) {
    const uint32_t a = (r & 1) | ((r >> 1) & l & 1), b = (r >> 1) & (l >> 1) & 1;
    return a | (b << 1);
  }
};
struct Sum {
  static constexpr uint32_t ident = 0;
  __device__ static uint32_t op(uint32_t l, uint32_t r) { return l + r; }
};

// Exclusive scan of one word per thread over the 1024-thread workgroup (op(l, r): l is
// the earlier operand). lds holds kTpWaves + 1 words.
template <typename Op>
__device__ __forceinline__ uint32_t tp_block_scan(uint32_t v, uint32_t* lds, uint32_t* total) {
  const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
  uint32_t x = v;
#pragma unroll
  for (int off = 1; off < 64; off <<= 1) {
    const uint32_t y = __shfl_up(x, off, 64);
    if (lane >= off) x = Op::op(y, x);
  }
  if (lane == 63) lds[wid] = x;
  __syncthreads();
  if (threadIdx.x == 0) {
    uint32_t run = Op::ident;
    for (int w = 0; w < kTpWaves; ++w) {
      const uint32_t t = lds[w];
      lds[w] = run;
      run = Op::op(run, t);
    }
    lds[kTpWaves] = run;
  }
  __syncthreads();
  uint32_t ex = __shfl_up(x, 1, 64);
  if (lane == 0) ex = Op::ident;
  const uint32_t res = Op::op(lds[wid], ex);
  *total = lds[kTpWaves];
  __syncthreads();
  return res;
}

// This thread's 16 bytes of the span at base into w (bytes past n read as '\n') and into
// lds_text; returns the byte before them ('\n' before the text). Ends behind a barrier: the
// whole span is in LDS.
__device__ __forceinline__ uint32_t tp_load_span(const uint8_t* __restrict__ text, int64_t n,
                                                 int64_t base, uint8_t* lds_text, uint32_t w[4]) {
  const int tid = threadIdx.x;
  const int64_t g0 = base + (int64_t)tid * kTpBytes;
  if (g0 + kTpBytes <= n) {
    const uint4 q = *reinterpret_cast<const uint4*>(text + g0);
    w[0] = q.x; w[1] = q.y; w[2] = q.z; w[3] = q.w;
  } else {
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      uint32_t x = 0;
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const int64_t g = g0 + k * 4 + j;
        x |= (uint32_t)(g < n ? text[g] : (uint8_t)'\n') << (8 * j);
      }
      w[k] = x;
    }
  }
  *reinterpret_cast<uint4*>(lds_text + tid * kTpBytes) = make_uint4(w[0], w[1], w[2], w[3]);
  __syncthreads();
  return tid > 0 ? lds_text[tid * kTpBytes - 1]
                 : (base > 0 ? (uint32_t)text[base - 1] : (uint32_t)'\n');
}

// The header of a chunk with `rows` rows and `nnz` features behind row0 / nnz0, the
// capacity check and the closing row offset (one thread, at the end of a scan launch).
__device__ __forceinline__ void tp_write_header(int64_t rows, int64_t nnz, uint32_t anom,
                                                int64_t row0, int64_t nnz0, int64_t cap_rows,
                                                int64_t cap_rp, int64_t cap_nnz,
                                                int64_t* __restrict__ row_ptr,
                                                int32_t* __restrict__ hdr) {
  const bool over = row0 + rows > cap_rows || row0 + rows + 1 > cap_rp || nnz0 + nnz > cap_nnz;
  hdr[H_ROWS] = (int32_t)rows;
  hdr[H_NNZ] = (int32_t)nnz;
  hdr[H_MINW] = INT32_MAX;
  hdr[H_MAXW] = 0;
  hdr[H_NONUNIT] = 0;
  hdr[H_BAD] = 0;
  hdr[H_DEFER] = (int32_t)anom;
  if (over) hdr[H_CAP] = 1;  // (sticky: only the caller clears it)
  else if (row_ptr) row_ptr[row0 + rows] = nnz0 + nnz;  // (model lines keep no offsets)
}

// The bytes of the token that starts at byte off of the span at base, and through *lim how
// many of them may be read: LDS when kMaxTok + 1 bytes from its start stay inside the span
// (bytes past n read as '\n' there), else global memory clamped to n.
__device__ __forceinline__ const uint8_t* tp_token_window(const uint8_t* __restrict__ text,
                                                          int64_t n, int64_t base, int off,
                                                          const uint8_t* lds_text, int* lim) {
  const int64_t left = n - (base + off);
  *lim = (int)(left < textnum::kMaxTok + 1 ? left : textnum::kMaxTok + 1);
  return off + textnum::kMaxTok + 1 <= kTpSpan ? lds_text + off : text + (base + off);
}

// Closes an emit launch: the per-workgroup reduction of the threads' bad / deferred tokens
// and "a value differs from 1" (kNonunit: the format has values); the header is touched only
// when there is something to add.
template <bool kNonunit = true>
__device__ __forceinline__ void tp_report(int bad, int defer, int nonunit,
                                          int32_t* __restrict__ hdr) {
  const int nbad = __syncthreads_count(bad), ndef = __syncthreads_count(defer);
  const int any_nu = kNonunit ? __syncthreads_or(nonunit) : 0;
  if (threadIdx.x == 0) {
    if (nbad) atomicAdd(&hdr[H_BAD], nbad);
    if (ndef) atomicAdd(&hdr[H_DEFER], ndef);
    if (any_nu && !__atomic_load_n(&hdr[H_NONUNIT], __ATOMIC_RELAXED)) atomicOr(&hdr[H_NONUNIT], 1);
  }
}

// Index order inside a row (LIBSVM) and the row-width range. A descent keys[j-1] > keys[j]
// is legal only where j starts a row: only descents search row_ptr (<= 40 bounded steps).
__global__ void __launch_bounds__(256) tp_finish_kernel(const uint64_t* __restrict__ keys,
                                                        const int64_t* __restrict__ row_ptr,
                                                        int64_t row0, int64_t nnz0, bool check_order,
                                                        int32_t* __restrict__ hdr) {
  __shared__ int32_t red[3][4];
  if (hdr[H_CAP]) return;
  const int64_t rows = hdr[H_ROWS], nnz = hdr[H_NNZ];
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  const int64_t t0 = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  int bad = 0;
  if (check_order) {
    for (int64_t j = t0 + 1; j < nnz; j += stride) {
      if (keys[nnz0 + j - 1] <= keys[nnz0 + j]) continue;
      const int64_t want = nnz0 + j;
      int64_t lo = 0, hi = rows;  // first r in [0, rows] with row_ptr[row0 + r] >= want
      for (int it = 0; it < 40 && lo < hi; ++it) {
        const int64_t mid = (lo + hi) >> 1;
        if (row_ptr[row0 + mid] < want) lo = mid + 1; else hi = mid;
      }
      if (row_ptr[row0 + lo] != want) ++bad;
    }
  }
  int32_t mn = INT32_MAX, mx = 0;
  for (int64_t q = t0; q < rows; q += stride) {
    const int64_t wd = row_ptr[row0 + q + 1] - row_ptr[row0 + q];
    const int32_t w32 = (int32_t)(wd < 0 ? 0 : (wd > INT32_MAX ? INT32_MAX : wd));
    mn = w32 < mn ? w32 : mn;
    mx = w32 > mx ? w32 : mx;
  }
  mn = wave_min(mn);
  mx = wave_max(mx);
  bad = wave_sum(bad);
  const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
  if (lane == 0) {
    red[0][wid] = mn;
    red[1][wid] = mx;
    red[2][wid] = bad;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    for (int w = 1; w < 4; ++w) {
      mn = red[0][w] < mn ? red[0][w] : mn;
      mx = red[1][w] > mx ? red[1][w] : mx;
      bad += red[2][w];
    }
    if (mn < __atomic_load_n(&hdr[H_MINW], __ATOMIC_RELAXED)) atomicMin(&hdr[H_MINW], mn);
    if (mx > __atomic_load_n(&hdr[H_MAXW], __ATOMIC_RELAXED)) atomicMax(&hdr[H_MAXW], mx);
    if (bad) atomicAdd(&hdr[H_BAD], bad);
  }
}

__global__ void __launch_bounds__(256) tp_mod_kernel(uint64_t* __restrict__ keys, int64_t nnz0,
                                                     uint64_t mod,
                                                     const int32_t* __restrict__ hdr) {
  if (hdr[H_CAP]) return;
  const int64_t nnz = hdr[H_NNZ];
  for (int64_t j = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; j < nnz;
       j += (int64_t)gridDim.x * blockDim.x)
    keys[nnz0 + j] %= mod;
}

inline int tp_fgrid(int64_t n) { return grid_for(n / 8 + 1, 256, 2048); }

// The launches that close every parser: tp_finish, then tp_mod when hash_mod is given.
inline void tp_finish(const TextOut& o, int64_t n, bool check_order, uint64_t hash_mod,
                      hipStream_t st) {
  const int fgrid = tp_fgrid(n);
  tp_finish_kernel<<<fgrid, 256, 0, st>>>(o.keys, o.row_ptr, o.row0, o.nnz0, check_order, o.hdr);
  if (hash_mod) tp_mod_kernel<<<fgrid, 256, 0, st>>>(o.keys, o.nnz0, hash_mod, o.hdr);
  PSAMD_HIP_CHECK(hipGetLastError());
}

}  // namespace

}  // namespace psamd
