// Forward / backward of a linear model on a "tp" or flat "tpf" localisation (localize_tp,
// localize_tpf), one 1024-thread workgroup per tile:
//   tp_bwd_accum*           backward alone: psum[tile entry] = sum over the tile's
//                           occurrences of the entry of coef[row] * val
//   tp_fwd_bwd_kernel       fused forward + tile backward, fixed row width 9..64
//   tp_fwd_bwd_csr_kernel   the same for variable-width / valued rows
//   tp_seg_reduce_kernel    compact layout: segmented scan of psum over the entry CSC -> grad
//   tp_seg_update_kernel    that scan fused with the 1-GPU optimizer update
// Every tile backward accumulates in 64-bit FIXED POINT with integer LDS atomics
// (tploc.cuh fx_shift / fx_add / fx_tile_max), never in float: exactly rounded,
// order-independent partials. On the flat layout the partials go to tploc_step.hip instead
// of the entry scan.
#include "tploc.cuh"
#include "tploc_geom.h"
#include "loss.cuh"

#include <stdexcept>

namespace psamd {

// Variable-width rows (rows != null): one LDS atomic per occurrence.
__global__ void __launch_bounds__(tp::kThr)
tp_bwd_accum_kernel(const uint16_t* __restrict__ rep, const int32_t* __restrict__ dcnt, int64_t n,
                    const int32_t* __restrict__ rows, int width, const float* __restrict__ vals,
                    const float* __restrict__ coef, int64_t B, float* __restrict__ psum) {
  using namespace tp;
  __shared__ long long acc[kTile];
  __shared__ uint32_t smax;
  const int t = threadIdx.x;
  for (int i = t; i < kTile; i += kThr) acc[i] = 0ll;
  if (t == 0) smax = 0u;
  const int64_t base = (int64_t)blockIdx.x * kTile;
  float v[kIt];
  uint16_t e[kIt];
  float vmax = 0.f;
#pragma unroll
  for (int j = 0; j < kIt; ++j) {
    const int64_t i = base + j * kThr + t;
    v[j] = 0.f;
    e[j] = 0;
    if (i < n) {
      const int64_t r = rows ? (int64_t)rows[i] : (int64_t)((uint32_t)i / (uint32_t)width);
      e[j] = rep[i];
      if (in_range(r, B)) v[j] = coef[r] * (vals ? vals[i] : 1.f);
    }
    vmax = fmaxf(vmax, fabsf(v[j]));
  }
  __syncthreads();  // acc / smax zeroed
  fx_tile_max(vmax, &smax);
  __syncthreads();
  const int k2 = fx_shift(smax);
  const double sc = ldexp(1.0, k2);
#pragma unroll
  for (int j = 0; j < kIt; ++j)
    if (v[j] != 0.f) fx_add(acc, e[j], v[j], sc);
  __syncthreads();
  const int cnt = min(kTile, max(0, dcnt[blockIdx.x]));
  const double isc = ldexp(1.0, -k2);
  for (int i = t; i < cnt; i += kThr) psum[base + i] = (float)((double)acc[i] * isc);
}

// Fixed-width rows: thread = (slot, run of L consecutive rows) walks down its column,
// so a hot key of a slot repeats along the walk and is summed in a register until the
// key changes (one LDS atomic per run instead of per occurrence); the lanes of a wave
// hold adjacent slots of the same rows, so the rep / vals loads stay coalesced.
// (Row-major lanes: LDS atomic waits on hot entries dominated, SQ_WAIT_INST_LDS.)
__global__ void __launch_bounds__(tp::kThr)
tp_bwd_accum_cols_kernel(const uint16_t* __restrict__ rep, const int32_t* __restrict__ dcnt,
                         int64_t n, int width, const float* __restrict__ vals,
                         const float* __restrict__ coef, int64_t B, float* __restrict__ psum) {
  using namespace tp;
  __shared__ long long acc[kTile];
  __shared__ uint32_t smax;
  const int t = threadIdx.x;
  for (int i = t; i < kTile; i += kThr) acc[i] = 0ll;
  if (t == 0) smax = 0u;
  const int64_t base = (int64_t)blockIdx.x * kTile;
  const int64_t lim = n - base < kTile ? n - base : kTile;
  const int64_t r0 = base / width, r1 = (base + lim - 1) / width;
  const int nr = (int)(r1 - r0 + 1);
  const int L = (nr * width + kThr - 1) / kThr;  // rows per thread
  const int nseg = (nr + L - 1) / L;
  const int slot = t % width, seg = t / width;
  const int ra = seg * L, rb = ra + L < nr ? ra + L : nr;
  constexpr int kL = 16;  // rows a thread prefetches into registers before its walk
  const bool regs = seg < nseg && L <= kL;
  uint32_t ee[kL];
  float vv[kL];
  float vmax = 0.f;
  if (regs) {
#pragma unroll
    for (int q = 0; q < kL; ++q) {  // every load of the walk in flight at once
      const int rl = ra + q;
      const int64_t r = r0 + rl;
      const int64_t i = r * width + slot;
      const bool ok = q < L && rl < nr && i >= base && i < base + lim && in_range(r, B);
      ee[q] = ok ? (uint32_t)rep[i] : 0xffffffffu;
      vv[q] = ok ? coef[r] * (vals ? vals[i] : 1.f) : 0.f;
      vmax = fmaxf(vmax, fabsf(vv[q]));
    }
  } else if (seg < nseg) {  // long walks (width > 1024 / kL rows): a max pre-pass
    for (int rl = ra; rl < rb; ++rl) {
      const int64_t r = r0 + rl;
      const int64_t i = r * width + slot;
      if (i >= base && i < base + lim && in_range(r, B))
        vmax = fmaxf(vmax, fabsf(coef[r] * (vals ? vals[i] : 1.f)));
    }
  }
  __syncthreads();  // acc / smax zeroed
  fx_tile_max(vmax, &smax);
  __syncthreads();
  const int k2 = fx_shift(smax);
  const double sc = ldexp(1.0, k2);
  uint32_t cur = 0xffffffffu;
  float sum = 0.f;  // a run of equal keys down the column (<= L addends < 2^e each)
  if (regs) {
#pragma unroll
    for (int q = 0; q < kL; ++q) {
      if (ee[q] == 0xffffffffu) continue;
      if (ee[q] != cur) {
        if (cur != 0xffffffffu && sum != 0.f) fx_add(acc, cur, sum, sc);
        cur = ee[q];
        sum = vv[q];
      } else {
        sum += vv[q];
      }
    }
  } else if (seg < nseg) {
    for (int rl = ra; rl < rb; ++rl) {
      const int64_t r = r0 + rl;
      const int64_t i = r * width + slot;  // global position
      if (i < base || i >= base + lim || !in_range(r, B)) continue;
      const uint32_t e = rep[i];
      const float v = coef[r] * (vals ? vals[i] : 1.f);
      if (e != cur) {
        if (cur != 0xffffffffu && sum != 0.f) fx_add(acc, cur, sum, sc);
        cur = e;
        sum = v;
      } else {
        sum += v;
      }
    }
  }
  if (cur != 0xffffffffu && sum != 0.f) fx_add(acc, cur, sum, sc);
  __syncthreads();
  const int cnt = min(kTile, max(0, dcnt[blockIdx.x]));
  const double isc = ldexp(1.0, -k2);
  for (int i = t; i < cnt; i += kThr) psum[base + i] = (float)((double)acc[i] * isc);
}

__global__ void __launch_bounds__(256)
tp_seg_reduce_kernel(const int32_t* __restrict__ pos_s, const int32_t* __restrict__ segid,
                     int64_t n_host, const int32_t* __restrict__ n_dev,
                     const float* __restrict__ psum, int64_t p_cap, float* __restrict__ grad,
                     int64_t grad_cap) {
  // segmented scan over the entry CSC on DPP lane moves (no ds_bpermute); run ends
  // store grad[u], runs cut by a wave boundary add atomically (grad zeroed by emit)
  const int lane = threadIdx.x & 63;
  const int64_t n = dev_len(n_dev, n_host);
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  for (int64_t i0 = blockIdx.x * (int64_t)blockDim.x + (threadIdx.x & ~63); i0 < n;
       i0 += stride) {
    const int64_t i = i0 + lane;
    const bool valid = i < n;
    int32_t s = -3;
    float x[1] = {0.f};
    if (valid) {
      s = segid[i];
      const int32_t p = pos_s[i];
      if (in_range(p, p_cap)) x[0] = psum[p];
    }
    const int32_t s_next = i + 1 < n ? segid[i + 1] : -1;
    const int32_t s_prev0 = i0 > 0 ? segid[i0 - 1] : -1;
    seg_scan_step<0x111, 0xf>(s, x);
    seg_scan_step<0x112, 0xf>(s, x);
    seg_scan_step<0x114, 0xf>(s, x);
    seg_scan_step<0x118, 0xf>(s, x);
    seg_scan_step<0x142, 0xa>(s, x);
    seg_scan_step<0x143, 0xc>(s, x);
    const int32_t s_lane0 = __builtin_amdgcn_readfirstlane(s);
    if (valid && (s_next != s || lane == 63)) {
      const bool starts_inside = s != s_lane0 || s_prev0 != s;
      const int32_t u = s - 1;
      if (in_range(u, grad_cap)) {
        if (starts_inside && s_next != s) grad[u] = x[0];
        else atomicAdd(&grad[u], x[0]);
      }
    }
  }
}

// Entry scan fused with the 1-GPU optimizer update (replaces tp_seg_reduce + kv_update:
// one launch and the grad[] round trip less). The segmented scan of tp_seg_reduce;
// a key whose entries all lie in one wave's 64-entry chunk has its full gradient in
// the lane that ends the run, which applies the update to the key's slot at once.
// A key spanning several chunks (hot keys: <= #tiles entries, so <= 6 chunks) adds
// each piece as ONE 64-bit integer atomic to acc[u] (zeroed by the bucket kernel):
// the piece in fixed point (scale 2^30) shifted left by 8, plus 1 in the low byte. The
// atomic returns the running (sum, count) together, so the piece that completes the
// count (chunks spanned, from seg_start) holds the whole sum and applies the update -
// no fence, no re-read (a device-scope __threadfence writes back the XCD's L2 and made
// a fence-based version 6x slower than the unfused pair). Binary features only (the
// host checks): |gradient| <= rows < 2^25 fits the 56-bit fixed-point field.
// Block 0 also turns the step's AUC histogram into metrics (as kv_update did).
__global__ void __launch_bounds__(256)
tp_seg_update_kernel(const int32_t* __restrict__ pos_s, const int32_t* __restrict__ segid,
                     int64_t n_host, const int32_t* __restrict__ n_dev,
                     const float* __restrict__ psum, int64_t p_cap,
                     const int32_t* __restrict__ seg_start, const int32_t* __restrict__ n_uniq,
                     unsigned long long* __restrict__ acc, int64_t u_cap,
                     const int64_t* __restrict__ slot_idx, Slot* __restrict__ slots, int64_t cap,
                     UpdateParams p, double* __restrict__ stats, int acc_stripes,
                     uint32_t* __restrict__ hist, int nbins, int hist_stripes,
                     double* __restrict__ metrics, int64_t* __restrict__ step_counter) {
  if (hist && blockIdx.x == 0) auc_hist_block(hist, nbins, hist_stripes, metrics, step_counter);
  const int lane = threadIdx.x & 63;
  const int64_t n = dev_len(n_dev, n_host);
  const int64_t U = dev_len(n_uniq, u_cap);
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  double dnnz = 0, wsum = 0, dsum = 0;
  for (int64_t i0 = blockIdx.x * (int64_t)blockDim.x + (threadIdx.x & ~63); i0 < n;
       i0 += stride) {
    const int64_t i = i0 + lane;
    const bool valid = i < n;
    int32_t s = -3;
    float x[1] = {0.f};
    if (valid) {
      s = segid[i];
      const int32_t q = pos_s[i];
      if (in_range(q, p_cap)) x[0] = psum[q];
    }
    const int32_t s_next = i + 1 < n ? segid[i + 1] : -1;
    const int32_t s_prev0 = i0 > 0 ? segid[i0 - 1] : -1;
    seg_scan_step<0x111, 0xf>(s, x);
    seg_scan_step<0x112, 0xf>(s, x);
    seg_scan_step<0x114, 0xf>(s, x);
    seg_scan_step<0x118, 0xf>(s, x);
    seg_scan_step<0x142, 0xa>(s, x);
    seg_scan_step<0x143, 0xc>(s, x);
    const int32_t s_lane0 = __builtin_amdgcn_readfirstlane(s);
    if (!(valid && (s_next != s || lane == 63))) continue;
    const int64_t u = (int64_t)s - 1;
    if (u < 0 || u >= U) continue;
    const bool starts_inside = s != s_lane0 || s_prev0 != s;
    float g = x[0];
    bool apply = starts_inside && s_next != s;
    if (!apply) {  // a piece of a key spanning several 64-entry chunks
      const long long fx = __double2ll_rn((double)g * 1073741824.0);  // 2^30
      const unsigned long long add = ((unsigned long long)fx << 8) + 1ull;
      const unsigned long long tot = atomicAdd(&acc[u], add) + add;
      const int64_t e0 = seg_start[u], e1 = seg_start[u + 1];
      const uint32_t np = (uint32_t)((e1 - 1) / 64 - e0 / 64 + 1);
      if ((uint32_t)(tot & 0xffull) == np) {
        g = (float)((double)((long long)tot >> 8) * (1.0 / 1073741824.0));
        apply = true;
      }
    }
    if (!apply) continue;
    const int64_t si = slot_idx[u];
    if (!in_range(si, cap)) continue;
    const float gs = g * p.grad_scale;
    if (gs != gs) continue;  // NaN mark = filtered entry
    Slot sl = slots[si];
    const float w_old = apply_update(sl, gs, p);
    slots[si] = sl;
    dnnz += (double)((sl.w != 0.f) - (w_old != 0.f));
    wsum += (double)sl.w * sl.w;
    const double d = (double)sl.w - w_old;
    dsum += d * d;
  }
  if (stats) {
    const double a = wave_sum_dpp(dnnz), b = wave_sum_dpp(wsum), c = wave_sum_dpp(dsum);
    if (lane == 63) {
      double* st = acc_stripe(stats, acc_stripes);
      if (a != 0) atomicAdd(&st[0], a);
      if (b != 0) atomicAdd(&st[1], b);
      if (c != 0) atomicAdd(&st[2], c);
    }
  }
}

// Fused forward + per-tile backward of a fixed-width linear model on a tp
// localisation, one workgroup per 8192-occurrence tile (replaces the local-column
// gather, linear_fwd and tp_bwd_accum: three launches and two global round trips).
// Every row overlapping the tile gets kFbLanes lanes strided over its occurrences.
//   prologue (all global loads in flight together): each lane's occurrences
//     (rep, val) into registers, the rows' labels into LDS, the tile's entry
//     weights wl[e] = w_local[ent_uid[tile + e]] into LDS; an occurrence of a row
//     cut by the tile boundary resolves its weight through the global entry map
//     and keeps w * val in its register slot;
//   forward: margins from registers + LDS, a DPP reduction per lane group into an LDS
//     row array; then ONE thread per row computes the loss terms (softplus, two expf
//     and two divides with the AUC bin: once per row, not in all 8 lanes of every
//     pass) and leaves the row's coef in its label slot, from where the lane groups
//     read it back (the tile holding a row's first occurrence owns its coef output,
//     metrics and AUC bin; the tile sums are DPP wave sums, the AUC bins a per-tile
//     LDS histogram). 65,536 x 39, flat: forward phase 11.9 k -> 7.7 k cycles per
//     workgroup, kernel 23.5 -> 20.5 us in the pipelined step
//     (profiles/r7_fused_rows.log);
//   backward: the same registers add coef * val into per-entry accumulators at rep,
//     then the per-entry partials psum[tile + e] go to tp_seg_reduce_kernel.
// The backward accumulates in 64-bit FIXED POINT with integer LDS atomics: on gfx950 a
// ds_add_f32 wave-instruction costs ~195 cycles whatever the addresses, ds_add_u64
// ~13-18 (benchmarks/micro/lds_atomics.hip, profiles/r2_lds_atomics.log), and the
// float atomics were 45 % of the kernel. The tile's scale 2^k (k = 48 - e, every
// |coef * val| < 2^e) keeps any sum of 8192 addends below 2^61 and quantises each
// addend at 2^-(k+1) relative to the tile's largest: the partials are the exactly
// rounded sums, independent of atomic order (deterministic).
// PER = occurrences per lane per row (width <= 8 * PER), NP = row passes held in
// registers (128 rows each): compile-time so the register slots stay registers.
constexpr int kFbLanes = 8;
constexpr int kFbMaxRows = tp::kTile / 8 + 2;  // width >= 8
constexpr int kFbMaxBins = 2048;                // AUC bins held in LDS (2 x 2048 u32)
constexpr uint16_t kFbNone = 0xffff, kFbExt = 0xfffe;

// Sum over the 8 lanes of an aligned lane group, result in all 8 (DPP: quad_perm
// [1,0,3,2], [2,3,0,1], then row_half_mirror; no LDS crossbar, bitwise equal in all 8).
__device__ __forceinline__ float group8_sum(float m) {
  m += __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(m), 0xB1, 0xf, 0xf, false));
  m += __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(m), 0x4E, 0xf, 0xf, false));
  m += __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(m), 0x141, 0xf, 0xf, false));
  return m;
}
// Sum over the wave in lane 63 (DPP row_shr 1/2/4/8, row_bcast:15 / :31, as
// wave_sum_dpp); the whole wave must be active.
__device__ __forceinline__ float fb_wave_sum(float v) {
#define PSAMD_FB_DPP(CTRL, ROWS) \
  v += __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(v), CTRL, ROWS, 0xf, false))
  PSAMD_FB_DPP(0x111, 0xf);
  PSAMD_FB_DPP(0x112, 0xf);
  PSAMD_FB_DPP(0x114, 0xf);
  PSAMD_FB_DPP(0x118, 0xf);
  PSAMD_FB_DPP(0x142, 0xa);
  PSAMD_FB_DPP(0x143, 0xc);
#undef PSAMD_FB_DPP
  return v;
}

// Phase marks of the fused kernel (a tuning aid, benchmarks/prof_tp_phases.py): null
// unless tp_fb_set_prof() installed a buffer of 16 u64 per workgroup.
__device__ uint64_t* g_fb_prof = nullptr;
#define FB_MARK(k)                                                             \
  if (fbp && threadIdx.x == 0) fbp[(int64_t)blockIdx.x * 16 + (k)] = clock64()

// kFlat (the flat 1-GPU path, tpf_step): w_local is already in tile-entry order
// (w_ent[tile * 8192 + e], scattered there by the step boundary kernel), so the
// prologue reads the tile's weights contiguously instead of the dependent
// ent_uid -> w_local gather (19 k of 37 k cycles per workgroup, r3_tp_pair_phases.log).
template <int PER, int NP, bool kFlat>
__global__ void __launch_bounds__(tp::kThr)  // 68 KB LDS -> 2 workgroups per CU
tp_fwd_bwd_kernel(const uint16_t* __restrict__ rep, const int32_t* __restrict__ dcnt,
                  const int32_t* __restrict__ ent_uid, int64_t n, int width,
                  const float* __restrict__ vals, const float* __restrict__ w_local, int64_t w_cap,
                  const float* __restrict__ labels, int64_t B, int loss_type,
                  float* __restrict__ coef_out, double* __restrict__ metrics,
                  uint32_t* __restrict__ hist, int nbins, int acc_stripes, int hist_stripes,
                  float* __restrict__ psum, int lts) {
  using namespace tp;
  // one 64 KB region: forward = entry weights (f32, [0, 32 KB)) + AUC histogram
  // ([32 KB, 48 KB)) + the rows' margins ([48 KB, 52 KB)); backward = the entries'
  // fixed-point accumulators (i64)
  __shared__ unsigned long long region[kTile];
  __shared__ float crow[kFbMaxRows];  // labels of the tile's rows, then their coefs
  __shared__ float sacc[3][kThr / 64];  // loss, correct, rows sums of every row wave
  __shared__ uint32_t smax;           // bits of the tile's largest |coef * val|
  float* const wl = reinterpret_cast<float*>(region);
  uint32_t* const lhist = reinterpret_cast<uint32_t*>(region) + kTile;
  float* const mrow = reinterpret_cast<float*>(region) + kTile + 2 * kFbMaxBins;
  static_assert(kTile + 2 * kFbMaxBins + kFbMaxRows <= 2 * kTile, "margins fit the region");
  long long* const acc = reinterpret_cast<long long*>(region);
  constexpr int kRowsPass = kThr / kFbLanes;
  const int t = threadIdx.x, sub = t % kFbLanes, g = t / kFbLanes;
  // occurrences [base, base + lim) (2^lts per tile), entries [eb, eb + cnt)
  const int64_t base = (int64_t)blockIdx.x << lts, eb = (int64_t)blockIdx.x * kTile;
  const int lim = (int)(n - base < (1 << lts) ? n - base : (1 << lts));
  const int64_t r0 = base / width;
  const int nr = (int)((base + lim - 1) / width - r0 + 1);
  const int cnt = min(kTile, max(0, dcnt[blockIdx.x]));
  uint64_t* const fbp = g_fb_prof;
  if (fbp && threadIdx.x == 0) fbp[(int64_t)blockIdx.x * 16 + 8] = __builtin_amdgcn_s_memrealtime();
  FB_MARK(0);
  uint16_t ce[NP][PER];
  float cv[NP][PER];
#pragma unroll
  for (int p = 0; p < NP; ++p) {
    const int ri = p * kRowsPass + g;
    const int64_t r = r0 + ri;
#pragma unroll
    for (int q = 0; q < PER; ++q) {
      const int k = sub + q * kFbLanes;
      ce[p][q] = kFbNone;
      cv[p][q] = 0.f;
      if (ri < nr && r < B && k < width) {
        const int64_t i = r * width + k;
        const int64_t o = i - base;
        const bool in = o >= 0 && o < lim;
        const uint16_t e = rep[i];  // outside the tile: the entry in the neighbour tile
        ce[p][q] = in ? e : kFbExt;
        cv[p][q] = in ? (vals ? vals[i] : 1.f) : __int_as_float((int)e);
      }
    }
  }
  if (t == 0) smax = 0u;
  // boundary rows: the outside part of row 0 / row nr-1 (only their lane groups) read
  // their weights through the neighbour tile's entry map; issued first, so the chain
  // rep -> ent_uid -> w_local overlaps the tile's own entry-weight loads
#pragma unroll
  for (int p = 0; p < NP; ++p) {
    const int ri = p * kRowsPass + g;
    if (ri != 0 && ri != nr - 1) continue;
#pragma unroll
    for (int q = 0; q < PER; ++q)
      if (ce[p][q] == kFbExt) {
        const int64_t i = (r0 + ri) * width + sub + q * kFbLanes;
        const int64_t ge = (i >> lts) * kTile + __float_as_int(cv[p][q]);
        const int64_t u = kFlat ? ge : (int64_t)ent_uid[ge];
        cv[p][q] = (in_range(u, w_cap) ? w_local[u] : 0.f) * (vals ? vals[i] : 1.f);
      }
  }
  for (int i = t; i < nr; i += kThr) crow[i] = r0 + i < B ? labels[r0 + i] : 0.f;
  if (kFlat) {
    for (int i = t; i < cnt; i += kThr) wl[i] = w_local[eb + i];  // (host: w_cap >= T * 8192)
  } else {
    for (int i = t; i < cnt; i += kThr) {
      const int32_t u = ent_uid[eb + i];
      wl[i] = in_range(u, w_cap) ? w_local[u] : 0.f;
    }
  }
  if (hist)
    for (int i = t; i < 2 * nbins; i += kThr) lhist[i] = 0u;
  __syncthreads();
  FB_MARK(1);
#pragma unroll
  for (int p = 0; p < NP; ++p) {
    float m = 0.f;
#pragma unroll
    for (int q = 0; q < PER; ++q) {
      const uint16_t e = ce[p][q];
      if (e == kFbExt) m += cv[p][q];
      else if (e != kFbNone) m += wl[e] * cv[p][q];
    }
    m = group8_sum(m);
    const int ri = p * kRowsPass + g;
    if (sub == 0 && ri < nr) mrow[ri] = m;
  }
  __syncthreads();
  FB_MARK(11);  // (forward = margins | row threads | coefs + tile max)
  // one thread per row: the loss terms once (not in all 8 lanes of every pass), the
  // row's coef into its label slot
  static_assert(NP * kRowsPass <= kThr, "a thread per row of the register passes");
  float loss_acc = 0.f, corr_acc = 0.f, rows_acc = 0.f;
  if (const int ri = t; ri < nr) {  // (host: nr <= NP * kRowsPass)
    const int64_t r = r0 + ri;
    float c = 0.f;
    if (r < B) {
      const float m = mrow[ri], lab = crow[ri];
      float loss, c2;
      loss_terms(m, lab, loss_type, loss, c, c2);
      if (r * width >= base) {  // first occurrence in this tile: the row is ours
        coef_out[r] = c;
        loss_acc += loss;
        corr_acc += ((lab > 0.f) == (m > 0.f)) ? 1.f : 0.f;
        rows_acc += 1.f;
        if (hist) atomicAdd(&lhist[auc_bin(m, lab, nbins)], 1u);
      }
    }
    crow[ri] = c;
  }
  // tile sums: a DPP sum per row wave into the wave's own slot, the slots summed by
  // wave 0 below. No float LDS atomics: with a thread per row, 3 ds_add_f32 of 64 lanes
  // on one address made the forward phase 11.9 k -> 19.8 k cycles (7.8 k with the DPP
  // sums, profiles/r7_fused_rows.log), and the tile's loss sum has a fixed order.
  if (metrics && (t & ~63) < nr) {
    loss_acc = fb_wave_sum(loss_acc);
    corr_acc = fb_wave_sum(corr_acc);
    rows_acc = fb_wave_sum(rows_acc);
    if ((t & 63) == 63) {
      sacc[0][t >> 6] = loss_acc;
      sacc[1][t >> 6] = corr_acc;
      sacc[2][t >> 6] = rows_acc;
    }
  }
  __syncthreads();
  FB_MARK(12);
  float cf[NP];  // every lane of a group holds its row's coef
  float vmax = 0.f;
#pragma unroll
  for (int p = 0; p < NP; ++p) {
    const int ri = p * kRowsPass + g;
    const float c = ri < nr ? crow[ri] : 0.f;
    cf[p] = c;
#pragma unroll
    for (int q = 0; q < PER; ++q)
      if (ce[p][q] < kFbExt) vmax = fmaxf(vmax, fabsf(c * cv[p][q]));
  }
  fx_tile_max(vmax, &smax);
  __syncthreads();
  FB_MARK(2);
  if (hist) {  // flush the AUC bins before the region turns into accumulators
    uint32_t* hs = hist + (int64_t)(blockIdx.x % hist_stripes) * 2 * nbins;
    for (int i = t; i < 2 * nbins; i += kThr)
      if (lhist[i]) atomicAdd(&hs[i], lhist[i]);
  }
  if (metrics && t < 64) {  // wave 0: lane w takes row wave w's sums, one more DPP sum
    const bool on = t * 64 < nr;
    const float ls = fb_wave_sum(on ? sacc[0][t] : 0.f);
    const float cs = fb_wave_sum(on ? sacc[1][t] : 0.f);
    const float rs = fb_wave_sum(on ? sacc[2][t] : 0.f);
    if (t == 63 && rs > 0.f) {
      double* mt = acc_stripe(metrics, acc_stripes);
      atomicAdd(&mt[0], (double)ls);
      atomicAdd(&mt[1], (double)cs);
      atomicAdd(&mt[2], (double)rs);
    }
  }
  const uint32_t mb = smax;
  __syncthreads();
  for (int i = t; i < cnt; i += kThr) acc[i] = 0ll;
  __syncthreads();
  FB_MARK(3);
  const int k2 = fx_shift(mb);  // every |addend| < 2^e -> scale 2^(48 - e)
  const double sc = ldexp(1.0, k2);
#pragma unroll
  for (int p = 0; p < NP; ++p) {
    if (cf[p] == 0.f) continue;
#pragma unroll
    for (int q = 0; q < PER; ++q)
      if (ce[p][q] < kFbExt) fx_add(acc, ce[p][q], cf[p] * cv[p][q], sc);  // ds_add_u64
  }
  FB_MARK(4);
  __syncthreads();
  FB_MARK(5);
  const double isc = ldexp(1.0, -k2);
  for (int i = t; i < cnt; i += kThr) psum[eb + i] = (float)((double)acc[i] * isc);
  FB_MARK(6);
  if (fbp && threadIdx.x == 0) {
    fbp[(int64_t)blockIdx.x * 16 + 9] = __builtin_amdgcn_s_memrealtime();
    fbp[(int64_t)blockIdx.x * 16 + 10] = __smid();
  }
}
#undef FB_MARK

// Variable-width / valued rows (CSR ``row_ptr`` + per-occurrence ``rows``, optional
// ``vals``; reference SparseMatrix::rangeTimes, src/util/sparse_matrix.h:73-107): the
// same fused forward + tile backward per 8192-occurrence tile as tp_fwd_bwd_kernel, for
// rows of any width. Thread t holds the tile's occurrences [8t, 8t+8) in registers
// (entry, value, row); a row's margin is summed in registers along the thread's run and
// added into an LDS row array once per run (rows of the tile: <= kCsrRows per window,
// windows repeat for tiles of very short rows). A row that starts before the tile or
// ends after it (the boundary rows) gets its outside part from one wave each, through
// the neighbour tiles' entry maps (flat: w_ent in tile-entry order). Every tile that
// holds part of a row computes that row's margin in full, so each uses the row's coef
// for its own entries; only the tile holding the row's first occurrence reports it
// (coef_out, loss, accuracy, AUC bin). Backward: 64-bit fixed point per tile entry
// (scale from the tile's largest |coef x val|), as the fixed-width kernel.
constexpr int kCsrRows = 4080;  // LDS row slots of one window (80 KB of LDS in all: 2 per CU)
// (~90 VGPRs: one workgroup per CU; a 64-VGPR bound spilled 100 B per lane. Real-data
// minibatches of this path are 10-600 tiles, so the grid rarely fills 2 per CU anyway.)
template <bool kFlat>
__global__ void __launch_bounds__(tp::kThr)
tp_fwd_bwd_csr_kernel(const uint16_t* __restrict__ rep, const int32_t* __restrict__ dcnt,
                      const int32_t* __restrict__ ent_uid, int64_t n,
                      const int64_t* __restrict__ row_ptr, const int32_t* __restrict__ rows,
                      const float* __restrict__ vals, const float* __restrict__ w_local,
                      int64_t w_cap, const float* __restrict__ labels, int64_t B, int loss_type,
                      float* __restrict__ coef_out, double* __restrict__ metrics,
                      uint32_t* __restrict__ hist, int nbins, int acc_stripes, int hist_stripes,
                      float* __restrict__ psum, int lts) {
  using namespace tp;
  __shared__ unsigned long long region[kTile];  // fwd: entry weights + AUC bins; bwd: i64 acc
  __shared__ float crow[kCsrRows];              // a window's row margins, then their coefs
  __shared__ float sacc[4];
  __shared__ float sc0;                         // coef of row r0 when an earlier tile owns it
  __shared__ uint32_t smax;
  float* const wl = reinterpret_cast<float*>(region);
  uint32_t* const lhist = reinterpret_cast<uint32_t*>(region) + kTile;
  long long* const acc = reinterpret_cast<long long*>(region);
  constexpr int kPer = kTile / kThr;  // 8 occurrences per thread
  constexpr uint32_t kNone = 0xffffffffu;
  const int t = threadIdx.x;
  // occurrences [base, base + lim) (2^lts per tile), entries [eb, eb + cnt)
  const int64_t base = (int64_t)blockIdx.x << lts, eb = (int64_t)blockIdx.x * kTile;
  const int lim = (int)(n - base < (1 << lts) ? n - base : (1 << lts));
  const int cnt = min(kTile, max(0, dcnt[blockIdx.x]));
  const int64_t r0 = rows[base], r1 = rows[base + lim - 1];  // (uniform loads)
  // occurrence = (row - r0) << 13 | tile entry (entries < 2^13; a tile's row span, empty
  // rows included, < 2^19 - 1: the host routes B >= kCsrMaxRows elsewhere)
  uint32_t er[kPer];
  float v[kPer];
  {  // 8 consecutive occurrences per thread: 16 / 32-byte loads, adjacent across lanes
    const int64_t i0 = base + (int64_t)t * kPer;
#pragma unroll
    for (int j = 0; j < kPer; ++j) {
      const bool in = t * kPer + j < lim;
      const int64_t i = in ? i0 + j : base;
      const uint32_t ee = rep[i];
      const int32_t rr = rows[i];
      er[j] = in ? (uint32_t)(rr - r0) << 13 | ee : kNone;
      v[j] = in ? (vals ? vals[i] : 1.f) : 0.f;
    }
  }
  const bool own0 = row_ptr[r0] >= base;
  if (t < 4) sacc[t] = 0.f;
  if (t == 0) smax = 0u;
  if (kFlat) {
    for (int i = t; i < cnt; i += kThr) wl[i] = w_local[eb + i];
  } else {
    for (int i = t; i < cnt; i += kThr) {
      const int32_t u = ent_uid[eb + i];
      wl[i] = in_range(u, w_cap) ? w_local[u] : 0.f;
    }
  }
  if (hist)
    for (int i = t; i < 2 * nbins; i += kThr) lhist[i] = 0u;
  const int wave = t / 64, lane = t % 64;
  const int nr = (int)(r1 - r0 + 1);
  float loss_acc = 0.f, corr_acc = 0.f, rows_acc = 0.f;
  for (int wa = 0; wa < nr; wa += kCsrRows) {  // row windows (1 unless rows are tiny)
    const int wb = min(nr, wa + kCsrRows);
    for (int i = t; i < wb - wa; i += kThr) crow[i] = 0.f;
    __syncthreads();
    {  // this thread's runs of equal rows -> one LDS add per run
      uint32_t cur = kNone;
      float sum = 0.f;
#pragma unroll
      for (int j = 0; j < kPer; ++j) {
        if (er[j] == kNone) continue;
        const uint32_t rr = er[j] >> 13;
        if (rr != cur) {
          if (cur != kNone && (int)cur >= wa && (int)cur < wb && sum != 0.f)
            atomicAdd(&crow[cur - wa], sum);
          cur = rr;
          sum = 0.f;
        }
        sum += wl[er[j] & 0x1fffu] * v[j];
      }
      if (cur != kNone && (int)cur >= wa && (int)cur < wb && sum != 0.f)
        atomicAdd(&crow[cur - wa], sum);
    }
    // boundary rows: wave 0 sums the part of row r0 before the tile, wave 1 the part of
    // row r1 after it (any length; a row longer than a tile has both)
    if (wave < 2) {
      const int rl = wave == 0 ? 0 : nr - 1;
      if (rl >= wa && rl < wb) {
        const int64_t r = r0 + rl;
        const int64_t a = wave == 0 ? row_ptr[r] : base + lim;
        const int64_t b = wave == 0 ? base : row_ptr[r + 1];
        float sum = 0.f;
        for (int64_t i = a + lane; i < b; i += 64) {
          const int64_t ge = (i >> lts) * kTile + (int64_t)rep[i];
          const int64_t u = kFlat ? ge : (int64_t)ent_uid[ge];
          sum += (in_range(u, w_cap) ? w_local[u] : 0.f) * (vals ? vals[i] : 1.f);
        }
        sum = wave_sum(sum);
        if (lane == 0 && sum != 0.f) atomicAdd(&crow[rl - wa], sum);
      }
    }
    __syncthreads();
    for (int i = t; i < wb - wa; i += kThr) {  // per row: loss terms -> coef
      const int64_t r = r0 + wa + i;
      float c = 0.f;
      if (r < B) {
        const float m = crow[i];
        const float lab = labels[r];
        float loss, c2;
        loss_terms(m, lab, loss_type, loss, c, c2);
        if (wa + i > 0 || own0) {  // the row's first occurrence is in this tile
          coef_out[r] = c;
          loss_acc += loss;
          corr_acc += ((lab > 0.f) == (m > 0.f)) ? 1.f : 0.f;
          rows_acc += 1.f;
          if (hist) atomicAdd(&lhist[auc_bin(m, lab, nbins)], 1u);
        } else {
          sc0 = c;
        }
      }
      crow[i] = c;
    }
    __syncthreads();
  }
  {  // empty rows (no occurrence) outside every tile's [first row, last row]: the gap
     // between the previous tile's last row and this tile's first (tile 0: from row 0)
     // and, in the last tile, the rows after its last one. Margin 0.
    const int64_t g0 = blockIdx.x == 0 ? 0 : (int64_t)rows[base - 1] + 1;
    const int64_t na = r0 > g0 ? r0 - g0 : 0;  // [g0, r0) (none when a row spans the cut)
    const int64_t nb = base + lim >= n && B > r1 + 1 ? B - (r1 + 1) : 0;  // (r1, B)
    for (int64_t i = t; i < na + nb; i += kThr) {
      const int64_t rr = i < na ? g0 + i : r1 + 1 + (i - na);
      const float lab = labels[rr];
      float loss, c, c2;
      loss_terms(0.f, lab, loss_type, loss, c, c2);
      coef_out[rr] = c;
      loss_acc += loss;
      corr_acc += (lab > 0.f) == false ? 1.f : 0.f;
      rows_acc += 1.f;
      if (hist) atomicAdd(&lhist[auc_bin(0.f, lab, nbins)], 1u);
    }
  }
  // coef of an occurrence's row: the window in LDS (one window), else the row's coef as
  // this workgroup wrote it to coef_out (sc0 for a row an earlier tile owns)
  const bool one = nr <= kCsrRows;
  auto coef_of = [&](uint32_t rr) -> float {
    if (one) return crow[rr];
    if (rr == 0 && !own0) return sc0;
    return coef_out[r0 + rr];
  };
  float vmax = 0.f;
#pragma unroll
  for (int j = 0; j < kPer; ++j)
    if (er[j] != kNone) vmax = fmaxf(vmax, fabsf(coef_of(er[j] >> 13) * v[j]));
  fx_tile_max(vmax, &smax);
  if (metrics && rows_acc > 0.f) {
    atomicAdd(&sacc[0], loss_acc);
    atomicAdd(&sacc[1], corr_acc);
    atomicAdd(&sacc[2], rows_acc);
  }
  __syncthreads();
  if (hist) {
    uint32_t* hs = hist + (int64_t)(blockIdx.x % hist_stripes) * 2 * nbins;
    for (int i = t; i < 2 * nbins; i += kThr)
      if (lhist[i]) atomicAdd(&hs[i], lhist[i]);
  }
  if (metrics && t == 0 && sacc[2] > 0.f) {
    double* mt = acc_stripe(metrics, acc_stripes);
    atomicAdd(&mt[0], (double)sacc[0]);
    atomicAdd(&mt[1], (double)sacc[1]);
    atomicAdd(&mt[2], (double)sacc[2]);
  }
  const uint32_t mb = smax;
  __syncthreads();
  for (int i = t; i < cnt; i += kThr) acc[i] = 0ll;
  __syncthreads();
  const int k2 = fx_shift(mb);
  const double sc = ldexp(1.0, k2);
#pragma unroll
  for (int j = 0; j < kPer; ++j)
    if (er[j] != kNone) {
      const float c = coef_of(er[j] >> 13);
      if (c != 0.f) fx_add(acc, er[j] & 0x1fffu, c * v[j], sc);
    }
  __syncthreads();
  const double isc = ldexp(1.0, -k2);
  for (int i = t; i < cnt; i += kThr) psum[eb + i] = (float)((double)acc[i] * isc);
}

void tp_fb_set_prof(uint64_t* p) {
  PSAMD_HIP_CHECK(hipMemcpyToSymbol(HIP_SYMBOL(g_fb_prof), &p, sizeof(p)));
}

// ------------------------------------------------------------------- host side
// the entry scan that ends every backward of the compact layout: psum -> grad
static void tp_seg_reduce(const TpGeom& g, const float* psum, const int32_t* pos_s,
                          const int32_t* segid, const int32_t* n_ent, float* grad,
                          int64_t grad_cap, hipStream_t st) {
  tp_seg_reduce_kernel<<<grid_for(g.N, 256, 2048), 256, 0, st>>>(pos_s, segid, g.N, n_ent, psum,
                                                                 g.N, grad, grad_cap);
  PSAMD_HIP_CHECK(hipGetLastError());
}

void tp_backward(const uint16_t* rep, const int32_t* dcnt, int64_t n, const int32_t* rows,
                 int width, const float* vals, const float* coef, int64_t B, float* psum,
                 const int32_t* pos_s, const int32_t* segid, const int32_t* n_ent, float* grad,
                 int64_t grad_cap, hipStream_t st) {
  if (n <= 0) return;
  const TpGeom g = tp_geom(n, 31);
  if (rows == nullptr && width >= 2 && width <= tp::kThr)
    tp_bwd_accum_cols_kernel<<<(unsigned)g.T, tp::kThr, 0, st>>>(rep, dcnt, n, width, vals, coef,
                                                                 B, psum);
  else
    tp_bwd_accum_kernel<<<(unsigned)g.T, tp::kThr, 0, st>>>(rep, dcnt, n, rows, width, vals, coef,
                                                            B, psum);
  PSAMD_HIP_CHECK(hipGetLastError());
  tp_seg_reduce(g, psum, pos_s, segid, n_ent, grad, grad_cap, st);
}

// register-held occurrences: PER = ceil(width / 8) in 2..8, NP = the row passes of
// the narrowest width with that PER (fewer register slots -> 2 workgroups per CU)
static int tp_fb_passes(int width) {
  return (int)((tp::kTile / width + 2 + tp::kThr / kFbLanes - 1) / (tp::kThr / kFbLanes));
}
static constexpr int kFbNP[9] = {0, 0, 8, 4, 3, 2, 2, 2, 2};

bool tp_fwd_bwd_supported(int width) {
  if (width < 9 || width > 64) return false;
  return tp_fb_passes(width) <= kFbNP[(width + kFbLanes - 1) / kFbLanes];
}

void tp_fwd_bwd(const uint16_t* rep, const int32_t* dcnt, const int32_t* ent_uid, int64_t n,
                int width, const float* vals, const float* w_local, int64_t w_cap,
                const float* labels, int64_t B, int loss_type, float* coef_out, double* metrics,
                uint32_t* hist, int nbins, int acc_stripes, int hist_stripes, float* psum,
                const int32_t* pos_s, const int32_t* segid, const int32_t* n_ent, float* grad,
                int64_t grad_cap, bool reduce, hipStream_t st) {
  if (n <= 0) return;
  if (!tp_fwd_bwd_supported(width) || n != B * (int64_t)width)
    throw std::runtime_error("tp_fwd_bwd: unsupported width or n != B * width");
  const bool flat = ent_uid == nullptr;  // w_local in tile-entry order (tpf)
  const TpGeom g = tp_geom(n, 31, flat);
  if (hist && (nbins <= 0 || nbins > kFbMaxBins))
    throw std::runtime_error("tp_fwd_bwd: 1..2048 AUC bins (LDS histogram)");
  const int per = (width + kFbLanes - 1) / kFbLanes;
  if (flat && w_cap < g.N) throw std::runtime_error("tp_fwd_bwd: flat w_ent < tile stride");
  // rows of one tile fit one register pass (<= 128 rows: 2^lts / width + 2): NP = 1
  const bool one = ((1 << g.lts) / width + 2) <= tp::kThr / kFbLanes;
#define PSAMD_FB(PER, NP)                                                                     \
  if (flat)                                                                                   \
    tp_fwd_bwd_kernel<PER, NP, true><<<(unsigned)g.T, tp::kThr, 0, st>>>(                    \
        rep, dcnt, ent_uid, n, width, vals, w_local, w_cap, labels, B, loss_type, coef_out,   \
        metrics, hist, nbins, acc_stripes, hist_stripes, psum, g.lts);                        \
  else                                                                                        \
    tp_fwd_bwd_kernel<PER, NP, false><<<(unsigned)g.T, tp::kThr, 0, st>>>(                   \
        rep, dcnt, ent_uid, n, width, vals, w_local, w_cap, labels, B, loss_type, coef_out,   \
        metrics, hist, nbins, acc_stripes, hist_stripes, psum, g.lts)
  if (one && flat) {
    switch (per) {
      case 2: PSAMD_FB(2, 1); break;
      case 3: PSAMD_FB(3, 1); break;
      case 4: PSAMD_FB(4, 1); break;
      case 5: PSAMD_FB(5, 1); break;
      case 6: PSAMD_FB(6, 1); break;
      case 7: PSAMD_FB(7, 1); break;
      default: PSAMD_FB(8, 1); break;
    }
  } else {
    switch (per) {  // NP = kFbNP[PER] row passes in registers (tp_fwd_bwd_supported)
      case 2: PSAMD_FB(2, 8); break;
      case 3: PSAMD_FB(3, 4); break;
      case 4: PSAMD_FB(4, 3); break;
      case 5: PSAMD_FB(5, 2); break;
      case 6: PSAMD_FB(6, 2); break;
      case 7: PSAMD_FB(7, 2); break;
      default: PSAMD_FB(8, 2); break;
    }
  }
#undef PSAMD_FB
  PSAMD_HIP_CHECK(hipGetLastError());
  // (reduce false: the caller runs tp_seg_update instead)
  if (reduce) tp_seg_reduce(g, psum, pos_s, segid, n_ent, grad, grad_cap, st);
}

void tp_fwd_bwd_csr(const uint16_t* rep, const int32_t* dcnt, const int32_t* ent_uid, int64_t n,
                    const int64_t* row_ptr, const int32_t* rows, const float* vals,
                    const float* w_local, int64_t w_cap, const float* labels, int64_t B,
                    int loss_type, float* coef_out, double* metrics, uint32_t* hist, int nbins,
                    int acc_stripes, int hist_stripes, float* psum, const int32_t* pos_s,
                    const int32_t* segid, const int32_t* n_ent, float* grad, int64_t grad_cap,
                    bool reduce, hipStream_t st) {
  if (n <= 0) return;
  const bool flat = ent_uid == nullptr;
  const TpGeom g = tp_geom(n, 31, flat);
  if (hist && (nbins <= 0 || nbins > kFbMaxBins))
    throw std::runtime_error("tp_fwd_bwd_csr: 1..2048 AUC bins (LDS histogram)");
  if (flat && w_cap < g.N) throw std::runtime_error("tp_fwd_bwd_csr: flat w_ent < tile stride");
  if (flat)
    tp_fwd_bwd_csr_kernel<true><<<(unsigned)g.T, tp::kThr, 0, st>>>(
        rep, dcnt, ent_uid, n, row_ptr, rows, vals, w_local, w_cap, labels, B, loss_type,
        coef_out, metrics, hist, nbins, acc_stripes, hist_stripes, psum, g.lts);
  else
    tp_fwd_bwd_csr_kernel<false><<<(unsigned)g.T, tp::kThr, 0, st>>>(
        rep, dcnt, ent_uid, n, row_ptr, rows, vals, w_local, w_cap, labels, B, loss_type,
        coef_out, metrics, hist, nbins, acc_stripes, hist_stripes, psum, g.lts);
  PSAMD_HIP_CHECK(hipGetLastError());
  if (reduce) tp_seg_reduce(g, psum, pos_s, segid, n_ent, grad, grad_cap, st);
}

void tp_seg_update(const int32_t* pos_s, const int32_t* segid, int64_t n, const int32_t* n_ent,
                   const float* psum, const int32_t* seg_start, const int32_t* n_uniq,
                   unsigned long long* acc, int64_t u_cap, const int64_t* slot_idx, void* slots,
                   int64_t cap, const UpdateParams& p, const StripedAcc& stats,
                   const AucOut& auc, hipStream_t st) {
  if (n <= 0) return;
  if (auc.hist && auc.nbins != 2048)
    throw std::runtime_error("tp_seg_update: the fused AUC needs 2048 bins");
  const TpGeom g = tp_geom(n, 31);
  tp_seg_update_kernel<<<grid_for(g.N, 256, 2048), 256, 0, st>>>(
      pos_s, segid, g.N, n_ent, psum, g.N, seg_start, n_uniq, acc, u_cap, slot_idx,
      (Slot*)slots, cap, p, stats.ptr, stats.stripes, auc.hist, auc.nbins, auc.stripes,
      auc.metrics, auc.step_counter);
  PSAMD_HIP_CHECK(hipGetLastError());
}

}  // namespace psamd
