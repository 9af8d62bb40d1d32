// The step boundary on the flat ("tpf") layout (localize_tpf writes it; its regions and
// the block -> group map are in tploc.cuh), one 256-thread workgroup per bucket group:
//   tpf_step_kernel        1 GPU: update the keys of minibatch A from its entry partials
//                          (64-bit fixed-point LDS sums), then pull minibatch B's keys
//                          from the table into its tile-entry order (w_ent)
//   tpf_pack_keys_kernel   multi-GPU padded exchange: every group's keys into its
//   tpf_unpack_w_kernel    owner's row, the pulled weights back into w_ent, the keys'
//   tpf_pack_grads_kernel  gradients (the same fixed-point sums) into the owner's row
// No group waits for another in any of them.
#include "tploc.cuh"
#include "loss.cuh"

#include <stdexcept>

namespace psamd {

// Lookup-or-insert of one key with ONE 16-B load per probe (key and weight of the slot
// together; resolve_key reads the weight after the key compare, a second round trip).
__device__ __forceinline__ uint32_t tpf_resolve(Slot* __restrict__ slots, uint64_t mask,
                                                uint64_t home_base, uint64_t home_m, int home_shr,
                                                uint64_t h, int init_type, float init_v,
                                                float init_s, uint64_t seed, float* w, int* ins) {
  uint64_t idx = home_slot(h, mask, home_base, home_m, home_shr) & mask;
  *w = 0.f;
  for (uint64_t probe = 0; probe <= mask; ++probe) {
    const uint4 v = *reinterpret_cast<const uint4*>(&slots[idx]);
    const uint64_t k = ((uint64_t)v.y << 32) | v.x;
    if (k == h) {  // (non-zero init: the weight once its inserter published it)
      *w = init_type == kInitZero ? __uint_as_float(v.z)
                                  : published_w(&slots[idx], h, init_type, init_v, init_s, seed);
      return (uint32_t)idx;
    }
    if (k == kEmptyKey) {
      const unsigned long long prev = atomicCAS((unsigned long long*)&slots[idx].key,
                                                (unsigned long long)kEmptyKey,
                                                (unsigned long long)h);
      if (prev == kEmptyKey) {
        if (init_type != kInitZero) {
          *w = init_value(h, init_type, init_v, init_s, seed);
          publish_init(&slots[idx], *w);
        }
        ++*ins;
        return (uint32_t)idx;
      }
      if (prev == h) {  // claimed by another lane meanwhile
        *w = published_w(&slots[idx], h, init_type, init_v, init_s, seed);
        return (uint32_t)idx;
      }
    }
    idx = (idx + 1) & mask;
  }
  return tpf::kNoSlot;
}

// The step boundary of the flat 1-GPU path, one 256-thread workgroup per bucket
// workgroup region (replaces tp_seg_update + kv_resolve: one launch, no global atomics):
//   update A   every unit: the entries' partials psum[ent_pos] go into per-key LDS
//              accumulators in 64-bit fixed point (scale 2^(48 - e) from the unit's
//              largest |partial| < 2^e: <= 8192 addends stay below 2^61; exact,
//              order-independent sums), then the optimizer update of each key at the
//              slot its pull resolved (slotA), with the update statistics
//   pull B     every unit: lookup-or-insert of B's keys -> slotB, weights into LDS, then
//              scattered to B's tile-entry order: w_ent[ent_pos] = w[ent_j]
// A and B must share the bucket geometry (same minibatch size); either half may be off
// (the first pull, the last update). Block 0 also turns A's AUC histogram into metrics.
// Within a workgroup the update's slot stores are visible to the pull's loads after the
// barrier (workgroup scope: same CU, write-through L1).
__global__ void __launch_bounds__(tpf::kThr)
tpf_step_kernel(int do_upd, const int32_t* __restrict__ cntA, const int32_t* __restrict__ posA,
                const uint16_t* __restrict__ jA, const uint32_t* __restrict__ slotA,
                const float* __restrict__ psum, int64_t p_cap, int do_res,
                const int32_t* __restrict__ cntB, const uint64_t* __restrict__ uniqB,
                const int32_t* __restrict__ posB, const uint16_t* __restrict__ jB,
                uint32_t* __restrict__ slotB, float* __restrict__ w_ent, int64_t w_cap,
                Slot* __restrict__ slots, uint64_t mask, uint64_t home_base, uint64_t home_m,
                int home_shr, int init_type, float init_v, float init_s, uint64_t seed,
                int32_t* __restrict__ err, int32_t* __restrict__ inserted, UpdateParams p,
                double* __restrict__ stats, int acc_stripes, uint32_t* __restrict__ hist,
                int nbins, int hist_stripes, double* __restrict__ metrics,
                int64_t* __restrict__ step_counter, int groups) {
  using namespace tpf;
  __shared__ long long acc[kUnitK];  // fixed-point gradient sums of a unit's keys
  __shared__ float wj[kUnitK];       // pulled weights of a unit's keys
  __shared__ uint32_t smax;
  const int t = threadIdx.x, lane = t & 63;
  // the step's AUC epilogue in an extra last workgroup of its own (tpf_step launches
  // groups + 1): in unit 0's workgroup its 8 dependent stripe loads delayed that unit
  if ((int)blockIdx.x >= groups) {
    if (do_upd && hist) auc_hist_block(hist, nbins, hist_stripes, metrics, step_counter);
    return;
  }
  const int b = tpf_xcd_group_of(blockIdx.x, groups);
  double dnnz = 0, wsum = 0, dsum = 0;
  if (do_upd) {
    const int32_t* c = cntA + (int64_t)b * 4;
#pragma unroll 1
    for (int s = 0; s < 2; ++s) {
      // (counts clamped to the regions: a corrupted count never leaves them)
      const int e0 = s ? min(max(c[1], 0), kEC) : 0;
      const int D = min(c[2 * s], kUnitK), E = min(c[2 * s + 1], kEC - e0);
      if (D <= 0) continue;
      const int64_t eb = (int64_t)b * kEC + e0;
      const int64_t kb = (int64_t)b * kUC + s * kUnitK;
      for (int j = t; j < D; j += kThr) acc[j] = 0ll;
      if (t == 0) smax = 0u;
      constexpr int kR = 8;  // entries held in registers per thread (<= 2048 per unit)
      float v[kR];
      uint16_t jj[kR];
      int32_t pos[kR];
      float vmax = 0.f;
      // two batches of unconditional loads at clamped in-region addresses (a guarded
      // load per entry compiled to a branch + s_waitcnt each: 2 x kR serialised round
      // trips), then selects
      const int64_t rb = (int64_t)b * kEC;  // (always inside the entry region)
#pragma unroll
      for (int r = 0; r < kR; ++r) {
        const int g = r * kThr + t;
        const int64_t gi = g < E ? eb + g : rb;
        pos[r] = posA[gi];
        jj[r] = jA[gi];
      }
#pragma unroll
      for (int r = 0; r < kR; ++r) {
        const bool ok = r * kThr + t < E && in_range(pos[r], p_cap);
        const float x = psum[ok ? pos[r] : 0];
        v[r] = ok ? x : 0.f;
        if (r * kThr + t >= E) jj[r] = 0;
      }
#pragma unroll
      for (int r = 0; r < kR; ++r) vmax = fmaxf(vmax, fabsf(v[r]));
      for (int g = kR * kThr + t; g < E; g += kThr) {
        const int32_t pos = posA[eb + g];
        if (in_range(pos, p_cap)) vmax = fmaxf(vmax, fabsf(psum[pos]));
      }
      __syncthreads();  // acc / smax zeroed
      fx_tile_max(vmax, &smax);
      __syncthreads();
      const int k2 = fx_shift(smax);
      const double sc = ldexp(1.0, k2);
#pragma unroll
      for (int r = 0; r < kR; ++r)
        if (v[r] != 0.f && jj[r] < kUnitK) fx_add(acc, jj[r], v[r], sc);
      for (int g = kR * kThr + t; g < E; g += kThr) {
        const int32_t pos = posA[eb + g];
        const uint16_t j = jA[eb + g];
        const float x = in_range(pos, p_cap) ? psum[pos] : 0.f;
        if (x != 0.f && j < kUnitK) fx_add(acc, j, x, sc);
      }
      __syncthreads();
      const double isc = ldexp(1.0, -k2);
      for (int j = t; j < D; j += kThr) {
        const uint32_t si = slotA[kb + j];
        if (si == kNoSlot || si > mask) continue;
        const float gs = (float)((double)acc[j] * isc) * p.grad_scale;
        if (gs != gs) continue;
        Slot sl = slots[si];
        const float w_old = apply_update(sl, gs, p);
        slots[si] = sl;
        dnnz += (double)((sl.w != 0.f) - (w_old != 0.f));
        wsum += (double)sl.w * sl.w;
        const double d = (double)sl.w - w_old;
        dsum += d * d;
      }
      __syncthreads();  // (acc of the next unit; the pull reads these slots)
    }
  }
  int ins = 0;
  if (do_res) {
    const int32_t* c = cntB + (int64_t)b * 4;
#pragma unroll 1
    for (int s = 0; s < 2; ++s) {
      const int e0 = s ? min(max(c[1], 0), kEC) : 0;
      const int D = min(c[2 * s], kUnitK), E = min(c[2 * s + 1], kEC - e0);
      if (D <= 0) continue;
      const int64_t eb = (int64_t)b * kEC + e0;
      const int64_t kb = (int64_t)b * kUC + s * kUnitK;
      for (int j = t; j < D; j += kThr) {
        float w;
        const uint32_t si = tpf_resolve(slots, mask, home_base, home_m, home_shr, uniqB[kb + j],
                                        init_type, init_v, init_s, seed, &w, &ins);
        if (si == kNoSlot && err) atomicOr(err, 1);  // table full
        slotB[kb + j] = si;
        wj[j] = w;
      }
      __syncthreads();
      const int64_t rb = (int64_t)b * kEC;
      for (int g0 = 0; g0 < E; g0 += 8 * kThr) {  // (8 entries per thread: loads batched)
        int32_t pp[8];
        uint16_t jq[8];
#pragma unroll
        for (int q = 0; q < 8; ++q) {
          const int g = g0 + q * kThr + t;
          const int64_t gi = g < E ? eb + g : rb;
          pp[q] = posB[gi];
          jq[q] = jB[gi];
        }
#pragma unroll
        for (int q = 0; q < 8; ++q)
          if (g0 + q * kThr + t < E && in_range(pp[q], w_cap) && jq[q] < kUnitK)
            w_ent[pp[q]] = wj[jq[q]];
      }
      __syncthreads();  // (wj of the next unit)
    }
  }
  if (do_upd && stats) {
    const double a = wave_sum_dpp(dnnz), bb = wave_sum_dpp(wsum), cc = wave_sum_dpp(dsum);
    if (lane == 63) {
      double* st = acc_stripe(stats, acc_stripes);
      if (a != 0) atomicAdd(&st[0], a);
      if (bb != 0) atomicAdd(&st[1], bb);
      if (cc != 0) atomicAdd(&st[2], cc);
    }
  }
  if (inserted) {
    const int tot = wave_sum(ins);
    if (lane == 0 && tot) atomicAdd(inserted, tot);
  }
}

// ---- the padded multi-GPU exchange on the flat layout (G peers, G a power of two that
// divides the bucket workgroups: owner p's key range is exactly the buckets
// [p * B / G, (p + 1) * B / G), whose keys are rank-sorted (tpf_bucket sorted = 1), so
// the rows stay key-ordered for the owner's partitioned apply). A bucket's keys sit in
// its owner's row after those of the owner's earlier buckets: that offset is the sum of
// < B / G earlier counts, read straight from cnt[] (the bucket kernel has completed),
// so no bucket waits for another.
__device__ __forceinline__ int tpf_row_base(const int32_t* __restrict__ cnt, int b, int per,
                                            uint32_t* red /* LDS [kThr/64 + 1] */) {
  const int b0 = (b / per) * per;
  int s = 0;
  for (int q = b0 + (int)threadIdx.x; q < b; q += blockDim.x) s += cnt[4 * q] + cnt[4 * q + 2];
  uint32_t tot;
  tp_block_scan<tpf::kThr>((uint32_t)s, red, &tot);
  return (int)tot;
}

// keys of every bucket into its owner's row of `send` ([nkeys, ngrads, -, - | keys (C x kw
// words) | grads]); the owner's last bucket writes the row's key count; keys past C
// count as overflow (ovf, once per owner)
// (the key of unit-concatenated index i of bucket b)
__device__ __forceinline__ uint64_t tpf_key_at(const uint64_t* __restrict__ uniqf, int b, int D0,
                                               int i) {
  return i < D0 ? uniqf[(int64_t)b * tpf::kUC + i]
                : uniqf[(int64_t)b * tpf::kUC + tpf::kUnitK + (i - D0)];
}

__global__ void __launch_bounds__(tpf::kThr)
tpf_pack_keys_kernel(const int32_t* __restrict__ cnt, const uint64_t* __restrict__ uniqf, int per,
                     int64_t C, int kw, int64_t H, int32_t* __restrict__ send,
                     int32_t* __restrict__ ovf) {
  using namespace tpf;
  __shared__ uint32_t red[kThr / 64 + 1];
  // (tpf_xcd_group_of: measured and not kept -- the keys are read contiguously per group)
  const int b = blockIdx.x, p = b / per, t = threadIdx.x;
  const int base = tpf_row_base(cnt, b, per, red);
  const int D0 = min(cnt[4 * b], kUnitK), D1 = min(cnt[4 * b + 2], kUnitK);
  int32_t* row = send + (int64_t)p * H;
  for (int i = t; i < D0 + D1; i += kThr) {
    const int64_t pos = (int64_t)base + i;
    if (pos >= C) break;
    const uint64_t k = tpf_key_at(uniqf, b, D0, i);
    if (kw == 1) row[4 + pos] = (int32_t)(uint32_t)k;
    else reinterpret_cast<uint64_t*>(row + 4)[pos] = k;
  }
  if (t == 0 && b % per == per - 1) {
    const int64_t tot = (int64_t)base + D0 + D1;
    row[0] = (int32_t)(tot < C ? tot : C);
    if (tot > C && ovf) atomicAdd(ovf, (int32_t)(tot - C));
  }
}

// pulled weights (row order, wrecv[p * C + i]) -> LDS per unit key -> the bucket's
// entries in tile-entry order (w_ent) for the flat fused forward
__global__ void __launch_bounds__(tpf::kThr)
tpf_unpack_w_kernel(const int32_t* __restrict__ cnt, const int32_t* __restrict__ ent_pos,
                    const uint16_t* __restrict__ ent_j, int per, int64_t C,
                    const float* __restrict__ wrecv, int64_t wstride, float* __restrict__ w_ent,
                    int64_t w_cap, int groups) {
  using namespace tpf;
  __shared__ uint32_t red[kThr / 64 + 1];
  __shared__ float wj[kUnitK];
  const int b = tpf_xcd_group_of(blockIdx.x, groups), p = b / per, t = threadIdx.x;
  const int base = tpf_row_base(cnt, b, per, red);
  const int32_t* c = cnt + 4 * b;
  int off = base;
#pragma unroll 1
  for (int s = 0; s < 2; ++s) {
    const int e0 = s ? min(max(c[1], 0), kEC) : 0;
    const int D = min(c[2 * s], kUnitK), E = min(c[2 * s + 1], kEC - e0);
    if (D <= 0) continue;
    for (int j = t; j < D; j += kThr) {
      const int64_t pos = (int64_t)off + j;
      wj[j] = pos < C ? wrecv[(int64_t)p * wstride + pos] : 0.f;
    }
    __syncthreads();
    const int64_t eb = (int64_t)b * kEC + e0, rb = (int64_t)b * kEC;
    for (int g0 = 0; g0 < E; g0 += 8 * kThr) {  // (8 entries per thread: loads batched)
      int32_t pp[8];
      uint16_t jq[8];
#pragma unroll
      for (int q = 0; q < 8; ++q) {
        const int g = g0 + q * kThr + t;
        const int64_t gi = g < E ? eb + g : rb;
        pp[q] = ent_pos[gi];
        jq[q] = ent_j[gi];
      }
#pragma unroll
      for (int q = 0; q < 8; ++q)
        if (g0 + q * kThr + t < E && in_range(pp[q], w_cap) && jq[q] < kUnitK)
          w_ent[pp[q]] = wj[jq[q]];
    }
    __syncthreads();
    off += D;
  }
}

// every key's gradient (its entries' partials summed in LDS, 64-bit fixed point as in
// tpf_step) into its owner's row; ff = 1: f32 into gstage[p * C + i] and the
// workgroup's FixingFloat min / max partial behind the rows (gstage[G * C + 2 b]), which
// xchg_ff_encode reduces per row. The owner's last bucket writes the row's gradient count.
// Block 0: the step's AUC epilogue and the overflow flag to the host.
__device__ __forceinline__ int tpf_ff_ord(float f) {
  const int b = __float_as_int(f);
  return b >= 0 ? b : b ^ 0x7fffffff;
}
__global__ void __launch_bounds__(tpf::kThr)
tpf_pack_grads_kernel(const int32_t* __restrict__ cnt, const int32_t* __restrict__ ent_pos,
                      const uint16_t* __restrict__ ent_j, int per, int64_t C, int kw, int64_t H,
                      const float* __restrict__ psum, int64_t p_cap, int32_t* __restrict__ send,
                      int ff, float* __restrict__ gstage, uint32_t* __restrict__ hist,
                      int hist_stripes, double* __restrict__ metrics,
                      int64_t* __restrict__ step_counter, const int32_t* __restrict__ ovf,
                      int32_t* __restrict__ ovf_host, int groups) {
  using namespace tpf;
  __shared__ uint32_t red[kThr / 64 + 1];
  __shared__ long long acc[kUnitK];
  __shared__ uint32_t smax;
  const int t = threadIdx.x, lane = t & 63;
  if ((int)blockIdx.x >= groups) {  // extra last workgroup (the launcher adds it)
    if (ovf_host && t == 0) ovf_host[0] = ovf[0];
    if (hist) auc_hist_block(hist, 2048, hist_stripes, metrics, step_counter);
    return;
  }
  const int b = tpf_xcd_group_of(blockIdx.x, groups), p = b / per;
  const int base = tpf_row_base(cnt, b, per, red);
  const int32_t* c = cnt + 4 * b;
  int32_t* row = send + (int64_t)p * H;
  float* grow = reinterpret_cast<float*>(row + 4 + C * kw);
  float lo = 3.4e38f, hi = -3.4e38f;
  int off = base;
#pragma unroll 1
  for (int s = 0; s < 2; ++s) {
    const int e0 = s ? min(max(c[1], 0), kEC) : 0;
    const int D = min(c[2 * s], kUnitK), E = min(c[2 * s + 1], kEC - e0);
    if (D <= 0) continue;
    const int64_t eb = (int64_t)b * kEC + e0;
    for (int j = t; j < D; j += kThr) acc[j] = 0ll;
    if (t == 0) smax = 0u;
    float vmax = 0.f;
    // the first 2048 entries' (pos, j) and partials in registers, loaded in two batches
    // at clamped in-region addresses (a guarded dependent load pair per entry compiled
    // to serialised round trips); the rest (rare) in a loop
    constexpr int kR = 8;
    const int64_t rb = (int64_t)b * kEC;
    int32_t pr[kR];
    uint16_t jr[kR];
    float xr[kR];
#pragma unroll
    for (int r = 0; r < kR; ++r) {
      const int g = r * kThr + t;
      const int64_t gi = g < E ? eb + g : rb;
      pr[r] = ent_pos[gi];
      jr[r] = ent_j[gi];
    }
#pragma unroll
    for (int r = 0; r < kR; ++r) {
      const bool ok = r * kThr + t < E && in_range(pr[r], p_cap);
      const float x = psum[ok ? pr[r] : 0];
      xr[r] = ok ? x : 0.f;
      vmax = fmaxf(vmax, fabsf(xr[r]));
    }
    for (int g = kR * kThr + t; g < E; g += kThr) {
      const int32_t pos = ent_pos[eb + g];
      if (in_range(pos, p_cap)) vmax = fmaxf(vmax, fabsf(psum[pos]));
    }
    __syncthreads();
    fx_tile_max(vmax, &smax);
    __syncthreads();
    const int k2 = fx_shift(smax);
    const double sc = ldexp(1.0, k2);
#pragma unroll
    for (int r = 0; r < kR; ++r)
      if (xr[r] != 0.f && jr[r] < kUnitK) fx_add(acc, jr[r], xr[r], sc);
    for (int g = kR * kThr + t; g < E; g += kThr) {
      const int32_t pos = ent_pos[eb + g];
      const uint16_t j = ent_j[eb + g];
      const float x = in_range(pos, p_cap) ? psum[pos] : 0.f;
      if (x != 0.f && j < kUnitK) fx_add(acc, j, x, sc);
    }
    __syncthreads();
    const double isc = ldexp(1.0, -k2);
    for (int j = t; j < D; j += kThr) {
      const int64_t pos = (int64_t)off + j;
      if (pos >= C) break;
      const float g = (float)((double)acc[j] * isc);
      if (ff) {
        gstage[(int64_t)p * C + pos] = g;
        if (g == g) {
          lo = fminf(lo, g);
          hi = fmaxf(hi, g);
        }
      } else {
        grow[pos] = g;
      }
    }
    __syncthreads();  // (acc of the next unit)
    off += D;
  }
  if (ff) {
    // the workgroup's min / max -> its partial at gstage[G * C + 2 b] (xchg_ff_encode
    // reduces a row's partials): per-wave atomics on the row header's two words were
    // ~8 k device-scope atomics on 16 addresses per step, serialised across the XCDs
    // (pack 16 -> 32 us with fixing-float at 8 emulated peers, gpurun r6u)
    lo = wave_min(lo);
    hi = wave_max(hi);
    __shared__ float sl[kThr / 64], sh[kThr / 64];
    if (lane == 0) {
      sl[t >> 6] = lo;
      sh[t >> 6] = hi;
    }
    __syncthreads();
    if (t == 0) {
      for (int w = 1; w < kThr / 64; ++w) {
        lo = fminf(lo, sl[w]);
        hi = fmaxf(hi, sh[w]);
      }
      float* part = gstage + (int64_t)(groups / per) * C;
      part[2 * b] = lo;
      part[2 * b + 1] = hi;
    }
  }
  if (t == 0 && b % per == per - 1) row[1] = (int32_t)(off < C ? off : C);
}

// multi-GPU flat exchange: the owner of bucket workgroup b is b / per, per = groups / G
bool tpf_exchange_ok(int64_t n, int bits, int G) {
  const int groups = tpf_groups(n, bits);
  return G >= 1 && !(G & (G - 1)) && groups % G == 0;
}
static int tpf_per_owner(int64_t n, int bits, int G) {
  if (!tpf_exchange_ok(n, bits, G))
    throw std::runtime_error("tpf exchange: G must be a power of two dividing the bucket groups");
  return tpf_groups(n, bits) / G;
}

void tpf_pack_keys(int64_t n, int bits, int G, const int32_t* cnt, const uint64_t* uniqf, int64_t C,
                   int kw, int64_t H, int32_t* send, int32_t* ovf, hipStream_t st) {
  const int per = tpf_per_owner(n, bits, G);
  tpf_pack_keys_kernel<<<(unsigned)tpf_groups(n, bits), tpf::kThr, 0, st>>>(
      cnt, uniqf, per, C, kw, H, send, ovf);
  PSAMD_HIP_CHECK(hipGetLastError());
}

void tpf_unpack_w(int64_t n, int bits, int G, const int32_t* cnt, const int32_t* ent_pos,
                  const uint16_t* ent_j, int64_t C, const float* wrecv, int64_t wstride,
                  float* w_ent, int64_t w_cap, hipStream_t st) {
  const int per = tpf_per_owner(n, bits, G);
  const int groups = tpf_groups(n, bits);
  tpf_unpack_w_kernel<<<(unsigned)groups, tpf::kThr, 0, st>>>(
      cnt, ent_pos, ent_j, per, C, wrecv, wstride > 0 ? wstride : C, w_ent, w_cap, groups);
  PSAMD_HIP_CHECK(hipGetLastError());
}

void tpf_pack_grads(int64_t n, int bits, int G, const int32_t* cnt, const int32_t* ent_pos,
                    const uint16_t* ent_j, int64_t C, int kw, int64_t H, const float* psum,
                    int64_t p_cap, int32_t* send, bool ff, float* gstage, const AucOut& auc,
                    const int32_t* ovf, int32_t* ovf_host, hipStream_t st) {
  const int per = tpf_per_owner(n, bits, G);
  // (+1 workgroup: the AUC epilogue / overflow publication, off unit 0's critical path)
  const int groups = tpf_groups(n, bits);
  tpf_pack_grads_kernel<<<(unsigned)groups + ((auc.hist || ovf_host) ? 1u : 0u), tpf::kThr, 0,
                          st>>>(cnt, ent_pos, ent_j, per, C, kw, H, psum, p_cap, send, ff ? 1 : 0,
                                gstage, auc.hist, auc.stripes, auc.metrics, auc.step_counter, ovf,
                                ovf_host, groups);
  PSAMD_HIP_CHECK(hipGetLastError());
}

// One launch of tpf_step_kernel over the groups of an n-key minibatch (A and B: the
// same n). A = null: pull only; B = null: update only.
void tpf_step(int64_t n, int bits, const int32_t* cntA, const int32_t* posA, const uint16_t* jA,
              const uint32_t* slotA, const float* psum, int64_t p_cap, const int32_t* cntB,
              const uint64_t* uniqB, const int32_t* posB, const uint16_t* jB, uint32_t* slotB,
              float* w_ent, int64_t w_cap, const TableRef& t, const KeyInit& init, int32_t* err,
              int32_t* inserted, const UpdateParams& p, const StripedAcc& stats,
              const AucOut& auc, hipStream_t st) {
  if (n <= 0) return;
  if (auc.hist && auc.nbins != 2048)
    throw std::runtime_error("tpf_step: the fused AUC needs 2048 bins");
  if (t.cap > (int64_t)1 << 32) throw std::runtime_error("tpf_step: > 2^32 slots (u32 slot ids)");
  int lg = 0;
  while ((1ll << lg) < t.cap) ++lg;
  const int groups = tpf_groups(n, bits);
  tpf_step_kernel<<<(unsigned)groups + (cntA && auc.hist ? 1u : 0u), tpf::kThr, 0, st>>>(
      cntA != nullptr, cntA, posA, jA, slotA, psum, p_cap, cntB != nullptr, cntB, uniqB, posB,
      jB, slotB, w_ent, w_cap, (Slot*)t.slots, (uint64_t)(t.cap - 1), t.home_base, t.home_m,
      64 - lg, init.type, init.v, init.s, init.seed, err, inserted, p, stats.ptr, stats.stripes,
      cntA ? auc.hist : nullptr, auc.nbins, auc.stripes, auc.metrics, auc.step_counter, groups);
  PSAMD_HIP_CHECK(hipGetLastError());
}

}  // namespace psamd
