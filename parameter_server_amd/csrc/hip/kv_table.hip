// HBM-resident sharded key/value store for scalar linear models.
//
// Replaces the reference's per-server CPU hash map `KVStore<K,V,E,S>`
// (src/parameter/kv_store.h:28-80) whose entries implement the optimizer
// (FTRLEntry / SGDEntry / AdaGradEntry, src/app/linear_method/async_sgd.h:71-124).
//
// Layout: open addressing, linear probing, one 32-byte slot per key
//   { u64 key(mixed) | f32 w | f32 z | f32 n | f32 acc | u32 cnt | u32 flags }
// so a lookup that hits on its first probe touches exactly one 32-B sector and
// the optimizer read-modify-write touches the same sector again. Probe index =
// fmix64(key) & mask. 10^9 keys at load 0.5 = 64 GB: fits one MI355X's 288 GB.
//
// Concurrency: a key transitions EMPTY -> key exactly once via 64-bit CAS, so
// a stale plain load can only return EMPTY (then the CAS is authoritative) or
// the final key. Payload updates to distinct slots are race free (callers
// dedupe keys per launch); cross-source duplicates are applied by sequential
// launches (reference semantics: every push message is one optimizer step)
// or by the accumulate/apply pair (synchronous / BSP aggregation).
#include "kv_table.h"
#include "kv_slot.cuh"
#include "loss.cuh"
#include <stdexcept>
#include <string>

namespace psamd {

__global__ void kv_init_kernel(Slot* __restrict__ slots, int64_t cap) {
  for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < cap;
       i += (int64_t)gridDim.x * blockDim.x) {
    Slot s;
    s.key = kEmptyKey;
    s.w = s.z = s.n = s.acc = 0.f;
    s.cnt = s.flags = 0;
    slots[i] = s;
  }
}

// Lookup (optionally insert) every key; write its slot index (-1 if absent or
// table full) and optionally its weight. The fused weight is exact for any init: a
// lane that finds a key another lane of this launch has just claimed reads the weight
// only once the inserter published it (kv_slot.cuh published_w), else the init value.
__global__ void kv_resolve_kernel(Slot* __restrict__ slots, uint64_t mask, uint64_t home_base,
                                  uint64_t home_m, int home_shr,
                                  const uint64_t* __restrict__ keys, int64_t n_host,
                                  const int32_t* __restrict__ n_dev,
                                  int64_t* __restrict__ out_slot, float* __restrict__ out_w,
                                  int insert, int init_type, float init_v, float init_s,
                                  uint64_t seed, int32_t* __restrict__ err,
                                  int32_t* __restrict__ inserted) {
  const int64_t n = dev_len(n_dev, n_host);
  int local_ins = 0;
  for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < n;
       i += (int64_t)gridDim.x * blockDim.x) {
    float w;
    const int64_t found = resolve_key(slots, mask, home_base, home_m, home_shr, keys[i], insert,
                                      init_type, init_v, init_s, seed, &w, &local_ins);
    if (found < 0 && insert && err) atomicOr(err, 1);  // table full
    out_slot[i] = found;
    if (out_w) out_w[i] = w;
  }
  if (inserted) {
    int tot = wave_sum(local_ins);
    if ((threadIdx.x & 63) == 0 && tot) atomicAdd(inserted, tot);
  }
}

// Owner side of the fixed-capacity exchange (exchange.hip): the received buffer
// holds one row of H int32 words per source rank, [nkeys, ngrads, -, -, keys (C x kw
// words), grads (C)]. blockIdx.y = source; resolves that row's nkeys keys into
// out_slot[s*C + i] and out_w[s*C + i] (the weights that travel back).
__global__ void kv_resolve_rows_kernel(Slot* __restrict__ slots, uint64_t mask,
                                       uint64_t home_base, uint64_t home_m, int home_shr,
                                       const int32_t* __restrict__ recv, int64_t H, int64_t C,
                                       int kw, int64_t* __restrict__ out_slot,
                                       float* __restrict__ out_w, int64_t wstride,
                                       int insert, int init_type,
                                       float init_v, float init_s, uint64_t seed,
                                       int32_t* __restrict__ err, int32_t* __restrict__ inserted,
                                       uint64_t* __restrict__ out_key, int32_t* __restrict__ bnd,
                                       int lgP) {
  const int s = blockIdx.y;
  const int32_t* row = recv + (int64_t)s * H;
  const int64_t n = dev_len(row, C);
  const int P = 1 << lgP;
  int32_t* rb = bnd ? bnd + (int64_t)s * (P + 1) : nullptr;
  if (rb && n == 0 && blockIdx.x == 0)
    for (int q = threadIdx.x; q <= P; q += blockDim.x) rb[q] = 0;
  int local_ins = 0;
  for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < n;
       i += (int64_t)gridDim.x * blockDim.x) {
    const uint64_t h = kw == 1 ? (uint64_t)(uint32_t)row[4 + i]
                               : reinterpret_cast<const uint64_t*>(row + 4)[i];
    float w;
    const int64_t found = resolve_key(slots, mask, home_base, home_m, home_shr, h, insert,
                                      init_type, init_v, init_s, seed, &w, &local_ins);
    if (found < 0 && insert && err) atomicOr(err, 1);
    out_slot[(int64_t)s * C + i] = found;
    out_w[(int64_t)s * wstride + i] = w;
    if (out_key) out_key[(int64_t)s * C + i] = h;
    if (rb) {  // partition bounds of this (sorted) row: rb[q] = #keys of partition < q
      const int q = key_part(h, home_base, home_m, lgP);
      int q0 = 0;
      if (i > 0) {
        const uint64_t hp = kw == 1 ? (uint64_t)(uint32_t)row[4 + i - 1]
                                    : reinterpret_cast<const uint64_t*>(row + 4)[i - 1];
        q0 = key_part(hp, home_base, home_m, lgP) + 1;
      }
      for (int j = q0; j <= q; ++j) rb[j] = (int32_t)i;
      if (i == n - 1)
        for (int j = q + 1; j <= P; ++j) rb[j] = (int32_t)n;
    }
  }
  if (inserted) {
    int tot = wave_sum(local_ins);
    if ((threadIdx.x & 63) == 0 && tot) atomicAdd(inserted, tot);
  }
}

// out[i] = slot.w (0 for missing), gathered by cached slot index.
__global__ void kv_gather_kernel(const Slot* __restrict__ slots, int64_t cap,
                                 const int64_t* __restrict__ slot_idx, int64_t n_host,
                                 const int32_t* __restrict__ n_dev, float* __restrict__ out,
                                 int field) {
  const int64_t n = dev_len(n_dev, n_host);
  for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < n;
       i += (int64_t)gridDim.x * blockDim.x) {
    const int64_t s = slot_idx[i];
    float v = 0.f;
    if (in_range(s, cap)) {
      const float* f = &slots[s].w;
      v = f[field];
    }
    out[i] = v;
  }
}

// Set fields (checkpoint restore / explicit assignment).
__global__ void kv_set_kernel(Slot* __restrict__ slots, int64_t cap,
                              const int64_t* __restrict__ slot_idx,
                              int64_t n, const float* __restrict__ w,
                              const float* __restrict__ z, const float* __restrict__ nn) {
  for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < n;
       i += (int64_t)gridDim.x * blockDim.x) {
    const int64_t s = slot_idx[i];
    if (!in_range(s, cap)) continue;
    if (w) publish_init(&slots[s], w[i]);  // (an explicit weight counts as published)
    if (z) slots[s].z = z[i];
    if (nn) slots[s].n = nn[i];
  }
}

// Apply one pushed gradient per (unique within this launch) slot.
// stats: [0] nnz delta (as double), [1] sum w_new^2, [2] sum (w_new-w_old)^2.
__global__ void kv_update_kernel(Slot* __restrict__ slots, int64_t cap,
                                 const int64_t* __restrict__ slot_idx,
                                 const float* __restrict__ grad, int64_t n_host,
                                 const int32_t* __restrict__ n_dev, UpdateParams p,
                                 double* __restrict__ stats, int acc_stripes,
                                 uint32_t* __restrict__ hist, int nbins, int hist_stripes,
                                 double* __restrict__ metrics, int64_t* __restrict__ step_counter) {
  // block 0 also turns the step's AUC histogram into metrics (the forward finished
  // before this launch): the separate single-block AUC launch leaves the critical path
  if (hist && blockIdx.x == 0) auc_hist_block(hist, nbins, hist_stripes, metrics, step_counter);
  const int64_t n = dev_len(n_dev, n_host);
  double dnnz = 0, wsum = 0, dsum = 0;
  for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < n;
       i += (int64_t)gridDim.x * blockDim.x) {
    const int64_t si = slot_idx[i];
    if (!in_range(si, cap)) continue;
    const float g = grad[i] * p.grad_scale;
    if (g != g) continue;  // NaN mark = filtered entry (reference SparseFilter)
    Slot s = slots[si];
    const float w_old = apply_update(s, g, p);
    slots[si] = s;
    dnnz += (double)((s.w != 0.f) - (w_old != 0.f));
    wsum += (double)s.w * s.w;
    const double d = (double)s.w - w_old;
    dsum += d * d;
  }
  if (stats) {  // per-wave DPP sums, lane 63 adds to the striped accumulators (no barriers)
    const double a = wave_sum_dpp(dnnz), b = wave_sum_dpp(wsum), c = wave_sum_dpp(dsum);
    if ((threadIdx.x & 63) == 63) {
      double* st = acc_stripe(stats, acc_stripes);
      if (a != 0) atomicAdd(&st[0], a);
      if (b != 0) atomicAdd(&st[1], b);
      if (c != 0) atomicAdd(&st[2], c);
    }
  }
}

// Synchronous aggregation: acc += g; the first toucher of a slot appends it to the
// touched list (one list atomic per wavefront, not per lane).
__device__ __forceinline__ void accumulate_one(Slot* __restrict__ slots, int64_t cap, int64_t si,
                                               float g, bool valid, int64_t* __restrict__ touched,
                                               int32_t* __restrict__ n_touched,
                                               int64_t touched_cap) {
  bool first = false;
  if (valid && in_range(si, cap) && g == g) {  // NaN mark = filtered entry
    atomicAdd(&slots[si].acc, g);
    first = atomicOr(&slots[si].flags, 1u) == 0u;
  }
  const uint64_t m = __ballot(first);
  if (!m) return;
  const int lane = threadIdx.x & 63;
  const int leader = __ffsll((long long)m) - 1;
  int base = 0;
  if (lane == leader) base = atomicAdd(n_touched, (int)__popcll(m));
  base = __shfl(base, leader, 64);
  if (first) {
    const int pos = base + (int)__popcll(m & ((1ull << lane) - 1ull));
    if (pos < touched_cap) touched[pos] = si;
  }
}

__global__ void kv_accumulate_kernel(Slot* __restrict__ slots, int64_t cap,
                                     const int64_t* __restrict__ slot_idx,
                                     const float* __restrict__ grad, int64_t n_host,
                                     const int32_t* __restrict__ n_dev,
                                     int64_t* __restrict__ touched, int32_t* __restrict__ n_touched,
                                     int64_t touched_cap) {
  const int64_t n = dev_len(n_dev, n_host);
  // whole wavefronts iterate together (the list append uses a ballot)
  for (int64_t i0 = blockIdx.x * (int64_t)blockDim.x + (threadIdx.x & ~63); i0 < n;
       i0 += (int64_t)gridDim.x * blockDim.x) {
    const int64_t i = i0 + (threadIdx.x & 63);
    const bool valid = i < n;
    accumulate_one(slots, cap, valid ? slot_idx[i] : -1, valid ? grad[i] : 0.f, valid, touched,
                   n_touched, touched_cap);
  }
}

// The owner's pushes of one step, all source rows in ONE launch (blockIdx.y = source):
// row s has ngrads = recv[s*H + 1] gradients at grad[s*gstride + i] for the slots
// slot_idx[s*C + i] resolved by that source's pull.
__global__ void kv_accumulate_rows_kernel(Slot* __restrict__ slots, int64_t cap,
                                          const int64_t* __restrict__ slot_idx,
                                          const float* __restrict__ grad, int64_t gstride,
                                          const int32_t* __restrict__ recv, int64_t H, int64_t C,
                                          int64_t* __restrict__ touched,
                                          int32_t* __restrict__ n_touched, int64_t touched_cap) {
  const int s = blockIdx.y;
  const int64_t n = dev_len(recv + (int64_t)s * H + 1, C);
  for (int64_t i0 = blockIdx.x * (int64_t)blockDim.x + (threadIdx.x & ~63); i0 < n;
       i0 += (int64_t)gridDim.x * blockDim.x) {
    const int64_t i = i0 + (threadIdx.x & 63);
    const bool valid = i < n;
    accumulate_one(slots, cap, valid ? slot_idx[(int64_t)s * C + i] : -1,
                   valid ? grad[(int64_t)s * gstride + i] : 0.f, valid, touched, n_touched,
                   touched_cap);
  }
}

__global__ void kv_apply_accumulated_kernel(Slot* __restrict__ slots, int64_t cap,
                                            const int64_t* __restrict__ touched,
                                            const int32_t* __restrict__ n_touched, int64_t max_n,
                                            UpdateParams p, double* __restrict__ stats,
                                            int acc_stripes) {
  const int64_t n = dev_len(n_touched, max_n);
  double dnnz = 0, wsum = 0, dsum = 0;
  for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < n;
       i += (int64_t)gridDim.x * blockDim.x) {
    const int64_t si = touched[i];
    if (!in_range(si, cap)) continue;
    Slot s = slots[si];
    const float g = s.acc * p.grad_scale;
    s.acc = 0.f;
    s.flags &= ~1u;  // (bit 1, the published-init mark, stays)
    const float w_old = apply_update(s, g, p);
    slots[si] = s;
    dnnz += (double)((s.w != 0.f) - (w_old != 0.f));
    wsum += (double)s.w * s.w;
    const double d = (double)s.w - w_old;
    dsum += d * d;
  }
  if (stats) {  // per-wave DPP sums, lane 63 adds to the striped accumulators (no barriers)
    const double a = wave_sum_dpp(dnnz), b = wave_sum_dpp(wsum), c = wave_sum_dpp(dsum);
    if ((threadIdx.x & 63) == 63) {
      double* st = acc_stripe(stats, acc_stripes);
      if (a != 0) atomicAdd(&st[0], a);
      if (b != 0) atomicAdd(&st[1], b);
      if (c != 0) atomicAdd(&st[2], c);
    }
  }
}

// ---------------------------------------------------------------------------
// The owner's pushes of one exchange, ALL G source rows, with per-push semantics
// (reference KVStore::setValue applies every push message as its own optimizer
// step, src/parameter/kv_store.h:47-57): a slot pushed by several sources gets
// their gradients one after the other in source-rank order. Instead of G
// launches (one per source row, the rows run in order), two launches for any G:
//   link:  each entry e = s*C + i (slot k) swaps itself into a per-exchange scratch
//          hash keyed by k (64-bit word = k << 32 | head entry) and keeps the
//          entry it replaced in nxt[e] -> one chain per slot, <= G entries long
//          (a source row holds distinct keys, so distinct slots);
//   apply: the entry that is the final head of its chain walks it, applies the
//          gradients in increasing entry order (= source order) to a register copy
//          of the slot and stores it once.
// Bitwise the same weights as the per-row launch sequence. Scratch: link[HS] u64
// (HS = power of two >= 2 * G * C), reset to ~0 by the launcher, nxt[G * C] i32.
constexpr int kMaxChain = 64;  // source rows per exchange (exchange.hip kMaxPeers)
__device__ __forceinline__ uint64_t link_probe_start(int64_t k, uint64_t hmask) {
  return fmix64((uint64_t)k) & hmask;
}

__global__ void kv_link_rows_kernel(const int64_t* __restrict__ slot_idx, int64_t cap,
                                    const float* __restrict__ grad, int64_t gstride,
                                    const int32_t* __restrict__ recv, int64_t H, int64_t C,
                                    unsigned long long* __restrict__ link, uint64_t hmask,
                                    int32_t* __restrict__ nxt) {
  const int s = blockIdx.y;
  const int64_t n = dev_len(recv + (int64_t)s * H + 1, C);
  for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < n;
       i += (int64_t)gridDim.x * blockDim.x) {
    const int64_t e = (int64_t)s * C + i;
    const int64_t k = slot_idx[e];
    const float g = grad[(int64_t)s * gstride + i];
    if (!in_range(k, cap) || g != g) continue;  // NaN mark = filtered entry
    uint64_t h = link_probe_start(k, hmask);
    for (uint64_t probe = 0; probe <= hmask; ++probe) {
      unsigned long long cur = link[h];
      bool done = false;
      while (true) {
        if (cur == ~0ull) {  // empty: claim it for k
          const unsigned long long mine = ((unsigned long long)k << 32) | (uint32_t)e;
          const unsigned long long prev = atomicCAS(&link[h], cur, mine);
          if (prev == cur) { nxt[e] = -1; done = true; break; }
          cur = prev;
          continue;
        }
        if ((int64_t)(cur >> 32) != k) break;  // another slot: next probe
        const unsigned long long mine = (cur & 0xffffffff00000000ull) | (uint32_t)e;
        const unsigned long long prev = atomicCAS(&link[h], cur, mine);
        if (prev == cur) { nxt[e] = (int32_t)(uint32_t)(cur & 0xffffffffull); done = true; break; }
        cur = prev;
      }
      if (done) break;
      h = (h + 1) & hmask;
    }
  }
}

__global__ void kv_apply_rows_kernel(Slot* __restrict__ slots, int64_t cap,
                                     const int64_t* __restrict__ slot_idx,
                                     const float* __restrict__ grad, int64_t gstride,
                                     const int32_t* __restrict__ recv, int64_t H, int64_t C,
                                     const unsigned long long* __restrict__ link, uint64_t hmask,
                                     const int32_t* __restrict__ nxt, int64_t n_ent,
                                     UpdateParams p, double* __restrict__ stats, int acc_stripes) {
  const int s = blockIdx.y;
  const int64_t n = dev_len(recv + (int64_t)s * H + 1, C);
  double dnnz = 0, wsum = 0, dsum = 0;
  for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < n;
       i += (int64_t)gridDim.x * blockDim.x) {
    const int64_t e = (int64_t)s * C + i;
    const int64_t k = slot_idx[e];
    const float g0 = grad[(int64_t)s * gstride + i];
    if (!in_range(k, cap) || g0 != g0) continue;
    uint64_t h = link_probe_start(k, hmask);
    unsigned long long cur = ~0ull;
    for (uint64_t probe = 0; probe <= hmask; ++probe) {
      cur = link[h];
      if (cur == ~0ull || (int64_t)(cur >> 32) == k) break;
      h = (h + 1) & hmask;
    }
    if (cur == ~0ull || (int64_t)(uint32_t)(cur & 0xffffffffull) != e) continue;  // not the head
    // chain length (<= number of source rows) and apply in increasing entry order
    int len = 0;
    for (int32_t c = (int32_t)e; c >= 0 && len < kMaxChain; c = nxt[c]) {
      if (!in_range((int64_t)c, n_ent)) break;
      ++len;
    }
    Slot sl = slots[k];
    int64_t last = -1;
    for (int it = 0; it < len; ++it) {
      int64_t best = INT64_MAX;
      int walked = 0;
      for (int32_t c = (int32_t)e; c >= 0 && walked < len; c = nxt[c], ++walked)
        if ((int64_t)c > last && (int64_t)c < best) best = c;
      if (best == INT64_MAX) break;
      const int64_t bs = best / C, bi = best - bs * C;
      const float g = grad[bs * gstride + bi] * p.grad_scale;
      const float w_old = apply_update(sl, g, p);
      dnnz += (double)((sl.w != 0.f) - (w_old != 0.f));
      wsum += (double)sl.w * sl.w;
      const double d = (double)sl.w - w_old;
      dsum += d * d;
      last = best;
    }
    slots[k] = sl;
  }
  if (stats) {  // per-wave DPP sums, lane 63 adds to the striped accumulators (no barriers)
    const double a = wave_sum_dpp(dnnz), b = wave_sum_dpp(wsum), c = wave_sum_dpp(dsum);
    if ((threadIdx.x & 63) == 63) {
      double* st = acc_stripe(stats, acc_stripes);
      if (a != 0) atomicAdd(&st[0], a);
      if (b != 0) atomicAdd(&st[1], b);
      if (c != 0) atomicAdd(&st[2], c);
    }
  }
}

// The same per-push semantics in ONE launch without global atomics or scratch
// resets, for shards with an ordered home whose source rows are sorted by key
// (the localisers' unique lists are): the resolve of the pull recorded each row's
// keys and the bounds of P = 2^lgP key-range partitions (kv_resolve_rows), so
// every partition is a run of consecutive entries in each row and no key spans
// two partitions. One workgroup per partition gathers its runs into LDS in
// windows of <= kApWin entries (a window ends at the smallest "last loaded key"
// of the rows that did not fit, so every key's entries share a window), chains
// entries of equal slot through an LDS hash, and the head of each chain applies
// its gradients in increasing entry order (= source-rank order) to a register
// copy of the slot: bitwise the weights of kv_apply_rows.
// (exchange.hip ff_unord: the order-preserving int of a FixingFloat row header -> float)
__device__ __forceinline__ float ff_unord_kv(int b) {
  return __int_as_float(b >= 0 ? b : b ^ 0x7fffffff);
}
constexpr int kApWin = 1024;   // entries per window
constexpr int kApRun = 16;     // a chain up to this long is ordered in LDS
constexpr int kApHash = 2048;  // LDS hash slots (power of two, >= 2 * kApWin)

// The body of kv_apply_part_kernel for partition blockIdx.x.
__device__ __forceinline__ void apply_part_block(
    Slot* __restrict__ slots, int64_t cap, const int64_t* __restrict__ slot_idx,
    const uint64_t* __restrict__ keys, const float* __restrict__ grad, int64_t gstride,
    const int32_t* __restrict__ recv, int64_t H, int64_t C, int G,
    const int32_t* __restrict__ bnd, int lgP, UpdateParams p, double* __restrict__ stats,
    int acc_stripes, int ffnb, int kw) {
  __shared__ uint32_t hk[kApHash];
  __shared__ int32_t hh[kApHash];
  __shared__ int32_t went[kApWin], wnx[kApWin], whs[kApWin];
  __shared__ float wg[kApWin];
  __shared__ int32_t wrun[256 * kApRun];  // per-thread chain runs (blockDim 256)
  __shared__ int32_t ra[kMaxChain], re[kMaxChain], roff[kMaxChain + 1], rcnt[kMaxChain];
  __shared__ uint64_t thk[kMaxChain];
  __shared__ uint64_t thr;
  const int tid = threadIdx.x, P = 1 << lgP, part = blockIdx.x;
  const int CH = max(1, kApWin / G);
  // ffnb > 0: the pushes are FixingFloat codes in the received rows, decoded here (the
  // math of xchg_ff_decode_kernel, bit for bit) instead of by a separate launch
  __shared__ double flo[kMaxChain], fbin[kMaxChain];
  const double fratio = ffnb ? (double)((1ull << (8 * ffnb)) - 2ull) : 1.0;
  if (ffnb && tid < G) {
    const int32_t* row = recv + (int64_t)tid * H;
    const float lo = ff_unord_kv(row[2]), hi = ff_unord_kv(row[3]) + 1e-6f;
    flo[tid] = lo;
    fbin[tid] = (double)hi - (double)lo;
  }
  if (tid < G) {
    const int32_t n = (int32_t)dev_len(recv + (int64_t)tid * H + 1, C);
    const int32_t* rb = bnd + (int64_t)tid * (P + 1);
    const int32_t a = min(rb[part], n), b = min(rb[part + 1], n);
    ra[tid] = a;
    re[tid] = max(a, b);
  }
  for (int h = tid; h < kApHash; h += blockDim.x) {
    hk[h] = 0xffffffffu;
    hh[h] = -1;
  }
  double dnnz = 0, wsum = 0, dsum = 0;
  for (;;) {
    __syncthreads();
    // the window's end keys of the rows that do not fit: one load per row, all rows in
    // parallel (a serial loop over the rows was a chain of up to G dependent global loads)
    if (tid < G) {
      const int rem = re[tid] - ra[tid];
      thk[tid] = rem > CH ? keys[(int64_t)tid * C + ra[tid] + CH - 1] : ~0ull;
      rcnt[tid] = 0;
    }
    __syncthreads();
    if (tid == 0) {
      int off = 0;
      uint64_t t = ~0ull;
      for (int s = 0; s < G; ++s) {
        roff[s] = off;
        off += min(re[s] - ra[s], CH);
        t = min(t, thk[s]);
      }
      roff[G] = off;
      thr = t;
    }
    __syncthreads();
    const int tot = roff[G];
    if (tot == 0) break;
    const uint64_t th = thr;
    for (int w = tid; w < tot; w += blockDim.x) {
      int lo = 0, hi = G - 1;  // row of window entry w: last s with roff[s] <= w
      while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if (roff[mid] <= w) lo = mid; else hi = mid - 1;
      }
      const int s = lo;
      const int64_t i = ra[s] + (w - roff[s]);
      const int64_t e = (int64_t)s * C + i;
      int32_t ent = -1;
      const uint64_t key = keys[e];  // three independent loads in flight together
      const int64_t k = slot_idx[e];
      float g;
      if (ffnb) {
        const uint8_t* code =
            reinterpret_cast<const uint8_t*>(recv + (int64_t)s * H + 4 + C * kw) + i * ffnb;
        uint64_t r = 0;
        for (int b = 0; b < ffnb; ++b) r |= (uint64_t)code[b] << (8 * b);
        g = (float)((double)r / fratio * fbin[s] + flo[s]);
      } else {
        g = grad[(int64_t)s * gstride + i];
      }
      if (key <= th) {
        atomicAdd(&rcnt[s], 1);
        if (in_range(k, cap) && g == g) {  // NaN mark = filtered entry
          const uint32_t ks = (uint32_t)k;
          uint32_t hp = (ks * 0x9E3779B1u) >> (32 - 11);  // log2(kApHash) = 11
          for (int probe = 0; probe < kApHash; ++probe) {
            const uint32_t prev = atomicCAS(&hk[hp], 0xffffffffu, ks);
            if (prev == 0xffffffffu || prev == ks) break;
            hp = (hp + 1) & (kApHash - 1);
          }
          ent = (int32_t)e;
          wg[w] = g;
          whs[w] = (int32_t)hp;
          wnx[w] = atomicExch(&hh[hp], w);
        }
      }
      went[w] = ent;
    }
    __syncthreads();
    for (int w = tid; w < tot; w += blockDim.x) {
      if (went[w] < 0 || hh[whs[w]] != w) continue;  // not the head of its chain
      const int64_t k = (int64_t)hk[whs[w]];
      Slot sl = slots[k];  // (the slot's load in flight while the chain is ordered)
      // the chain (keys shared by several source rows: hot features) into this thread's
      // LDS run, insertion-sorted by entry (= source-rank) order: one pointer chase and
      // ~len^2 / 4 compares, instead of a full chain walk per applied entry (len^2
      // dependent LDS reads: 64 for a key in all 8 rows of an 8-peer exchange)
      int32_t* run = wrun + tid * kApRun;
      int len = 0;
      int c = w;
      for (; c >= 0 && len < kApRun; c = wnx[c]) {
        const int32_t e = went[c];
        int q = len++;
        for (; q > 0 && went[run[q - 1]] > e; --q) run[q] = run[q - 1];
        run[q] = c;
      }
      if (c < 0) {
        for (int it = 0; it < len; ++it) {
          const int bw = run[it];
          const float w_old = apply_update(sl, wg[bw] * p.grad_scale, p);
          dnnz += (double)((sl.w != 0.f) - (w_old != 0.f));
          wsum += (double)sl.w * sl.w;
          const double d = (double)sl.w - w_old;
          dsum += d * d;
        }
      } else {  // (a longer chain: the selection walk)
        len = 0;
        for (int cc = w; cc >= 0 && len < kMaxChain; cc = wnx[cc]) ++len;
        int32_t last = -1;
        for (int it = 0; it < len; ++it) {  // next entry in increasing (source) order
          int32_t best = INT32_MAX, bw = -1, walked = 0;
          for (int cc = w; cc >= 0 && walked < len; cc = wnx[cc], ++walked)
            if (went[cc] > last && went[cc] < best) { best = went[cc]; bw = cc; }
          if (bw < 0) break;
          const float w_old = apply_update(sl, wg[bw] * p.grad_scale, p);
          dnnz += (double)((sl.w != 0.f) - (w_old != 0.f));
          wsum += (double)sl.w * sl.w;
          const double d = (double)sl.w - w_old;
          dsum += d * d;
          last = best;
        }
      }
      slots[k] = sl;
    }
    __syncthreads();
    if (tid < G) ra[tid] += rcnt[tid];
    for (int h = tid; h < kApHash; h += blockDim.x) {
      hk[h] = 0xffffffffu;
      hh[h] = -1;
    }
  }
  if (stats) {  // per-wave DPP sums, lane 63 adds to the striped accumulators (no barriers)
    const double a = wave_sum_dpp(dnnz), b = wave_sum_dpp(wsum), c = wave_sum_dpp(dsum);
    if ((threadIdx.x & 63) == 63) {
      double* st = acc_stripe(stats, acc_stripes);
      if (a != 0) atomicAdd(&st[0], a);
      if (b != 0) atomicAdd(&st[1], b);
      if (c != 0) atomicAdd(&st[2], c);
    }
  }
}

__global__ __launch_bounds__(256) void kv_apply_part_kernel(
    Slot* __restrict__ slots, int64_t cap, const int64_t* __restrict__ slot_idx,
    const uint64_t* __restrict__ keys, const float* __restrict__ grad, int64_t gstride,
    const int32_t* __restrict__ recv, int64_t H, int64_t C, int G,
    const int32_t* __restrict__ bnd, int lgP, UpdateParams p, double* __restrict__ stats,
    int acc_stripes, int ffnb, int kw) {
  apply_part_block(slots, cap, slot_idx, keys, grad, gstride, recv, H, C, G, bnd, lgP, p, stats,
                   acc_stripes, ffnb, kw);
}

// Occupancy / sparsity census: out[0] = occupied slots, out[1] = nonzero w.
__global__ void kv_census_kernel(const Slot* __restrict__ slots, int64_t cap,
                                 unsigned long long* __restrict__ out) {
  unsigned long long occ = 0, nz = 0;
  for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < cap;
       i += (int64_t)gridDim.x * blockDim.x) {
    const uint64_t k = slots[i].key;
    if (k != kEmptyKey) {
      ++occ;
      nz += slots[i].w != 0.f;
    }
  }
  occ = wave_sum(occ);
  nz = wave_sum(nz);
  if ((threadIdx.x & 63) == 0) {
    if (occ) atomicAdd(&out[0], occ);
    if (nz) atomicAdd(&out[1], nz);
  }
}

// Growth: move every occupied slot of `old_slots` into the larger, freshly initialised
// `slots` (kv_init ran in a launch of its own). The whole 32-byte record travels
// unchanged; its new home is home_slot for the new capacity, claimed by CAS
// kEmptyKey -> key with linear probing exactly as resolve_key inserts, so the new probe
// chains have no gaps. Nothing reads the new table during the launch: the payload is a
// plain store behind the claim. moved[] is a striped counter (acc_stripe layout, one
// atomic per block); the launcher's caller sums it, so a growth needs no census.
__global__ __launch_bounds__(256) void kv_rehash_kernel(
    const Slot* __restrict__ old_slots, int64_t old_cap, Slot* __restrict__ slots, uint64_t mask,
    uint64_t home_base, uint64_t home_m, int home_shr, unsigned long long* __restrict__ moved,
    int stripes, int32_t* __restrict__ err) {
  __shared__ int wcnt[4];
  int cnt = 0;
  for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < old_cap;
       i += (int64_t)gridDim.x * blockDim.x) {
    const Slot s = old_slots[i];
    if (s.key == kEmptyKey) continue;
    uint64_t idx = home_slot(s.key, mask, home_base, home_m, home_shr) & mask;
    bool placed = false;
    for (uint64_t probe = 0; probe <= mask; ++probe) {
      if (slots[idx].key == kEmptyKey &&
          atomicCAS((unsigned long long*)&slots[idx].key, (unsigned long long)kEmptyKey,
                    (unsigned long long)s.key) == kEmptyKey) {
        Slot* d = &slots[idx];
        d->w = s.w;
        d->z = s.z;
        d->n = s.n;
        d->acc = s.acc;
        d->cnt = s.cnt;
        d->flags = s.flags;
        placed = true;
        break;
      }
      idx = (idx + 1) & mask;
    }
    if (placed) ++cnt;
    else if (err) atomicOr(err, 1);  // new table exhausted (never when new cap >= old cap)
  }
  cnt = wave_sum(cnt);
  if ((threadIdx.x & 63) == 0) wcnt[threadIdx.x >> 6] = cnt;
  __syncthreads();
  if (threadIdx.x == 0) {
    const int tot = wcnt[0] + wcnt[1] + wcnt[2] + wcnt[3];
    if (tot) atomicAdd(&moved[(int64_t)(blockIdx.x % stripes) * kAccStride], (unsigned long long)tot);
  }
}

// Warm start: seed a parsed chunk of a key<TAB>weight model file into the live table with
// the optimizer state that REPRODUCES each weight (a table loaded with w and z = n = 0
// forgets the weight at the key's first FTRL update: z += g - sigma * w_old, w = prox(-z eta)).
//   inv_eta0 = 1 / alpha (constant) or (n0 + beta) / alpha (decay); never 1 / eta, so that
//              beta = n0 = 0 gives 0 and not a division by zero
//   FTRL:    n = n0, z = -(w * (inv_eta0 + l2) + copysign(l1, w))   (the inverse of
//            soft_threshold_prox(-z eta0, eta0, l1, l2); every term has the sign of w)
//   AdaGrad: z = 0, n = n0^2.   SGD: z = n = 0 (cnt = 0).
// Per entry: a raw key outside [0, 2^bits) is counted and dropped, the key is mixed, kept
// when its mixed value lies in [lo, last] (this shard's range), dropped when w is 0 or NaN,
// then looked up or inserted by resolve_key's rules (the table's own home map, CAS claim,
// trip bound mask + 1, err bit 0 when the table is full) and the WHOLE slot is written as
// two 16-byte stores: {key, w (the file's bits), z} and {n, acc = 0, cnt = 0, kSlotInit}.
//
// The probes are random 32-byte lines and latency bound (as predict.hip): a thread takes
// kSeedBatch entries per round and issues all their first probes -- one 16-byte load of
// {key, w, z} at a clamped, in-range address for entries past the end -- before it looks at
// any. A stale first probe can only read kEmptyKey for a slot claimed meanwhile; the CAS
// decides. The kernel runs alone on the table (the caller flushed; no step in flight).
// counts: striped u64 (acc_stripe layout) [seeded, overwritten, foreign, out_of_range,
// skipped]; stats[0] += the change of the table's non-zero weight count.
constexpr int kSeedBatch = 4;
enum SeedCount : int { kSeedNew = 0, kSeedOver, kSeedForeign, kSeedRange, kSeedSkip, kSeedCounts };

__global__ __launch_bounds__(256) void kv_seed_kernel(
    Slot* __restrict__ slots, uint64_t mask, uint64_t home_base, uint64_t home_m, int home_shr,
    KeyMix km, const uint64_t* __restrict__ raw, const float* __restrict__ wv, int64_t n,
    uint64_t lo, uint64_t last, UpdateParams p, float n0,
    unsigned long long* __restrict__ counts, int count_stripes, double* __restrict__ stats,
    int acc_stripes, int32_t* __restrict__ err) {
  const float inv_eta0 = p.lr_type == kLrConstant ? 1.f / p.alpha : (n0 + p.beta) / p.alpha;
  const float zscale = inv_eta0 + p.l2;
  const float n_seed = p.algo == kFTRL ? n0 : (p.algo == kAdaGrad ? n0 * n0 : 0.f);
  int c_new = 0, c_over = 0, c_foreign = 0, c_range = 0, c_skip = 0, dnnz = 0;
  const int64_t threads = (int64_t)gridDim.x * blockDim.x;
  for (int64_t i0 = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i0 < n;
       i0 += threads * kSeedBatch) {
    uint64_t h[kSeedBatch], idx[kSeedBatch];
    float w[kSeedBatch];
    uint4 v[kSeedBatch];
    bool act[kSeedBatch];
#pragma unroll
    for (int j = 0; j < kSeedBatch; ++j) {
      const int64_t i = i0 + j * threads;
      const bool ok = i < n;
      const int64_t ic = ok ? i : n - 1;  // (n > 0 here: i0 < n)
      const uint64_t r = raw[ic];
      w[j] = wv[ic];
      h[j] = mix_key(r, km);
      const bool in_bits = r <= km.mask;
      const bool owned = h[j] >= lo && h[j] <= last;
      const bool keep = w[j] != 0.f && w[j] == w[j];
      act[j] = ok && in_bits && owned && keep;
      c_range += ok && !in_bits;
      c_foreign += ok && in_bits && !owned;
      c_skip += ok && in_bits && owned && !keep;
    }
#pragma unroll
    for (int j = 0; j < kSeedBatch; ++j) {
      idx[j] = home_slot(h[j], mask, home_base, home_m, home_shr) & mask;
      v[j] = *reinterpret_cast<const uint4*>(slots + idx[j]);
    }
#pragma unroll
    for (int j = 0; j < kSeedBatch; ++j) {
      if (!act[j]) continue;
      uint64_t at = idx[j];
      uint64_t k = ((uint64_t)v[j].y << 32) | v[j].x;
      float w_old = __uint_as_float(v[j].z);
      bool found = false, fresh = false;
      for (uint64_t probe = 0; probe <= mask; ++probe) {  // TRIP BOUND: mask + 1 slots
        if (probe) {
          k = slots[at].key;
          w_old = slots[at].w;
        }
        if (k == kEmptyKey) {
          k = atomicCAS((unsigned long long*)&slots[at].key, (unsigned long long)kEmptyKey,
                        (unsigned long long)h[j]);
          if (k == kEmptyKey) {
            found = fresh = true;
            break;
          }
          w_old = 0.f;  // (claimed meanwhile: by this launch, counted as a repeat if k == h)
        }
        if (k == h[j]) {
          found = true;
          break;
        }
        at = (at + 1) & mask;
      }
      if (!found) {
        if (err) atomicOr(err, 1);  // table full
        continue;
      }
      const float z = p.algo == kFTRL ? -(w[j] * zscale + copysignf(p.l1, w[j])) : 0.f;
      uint4* d = reinterpret_cast<uint4*>(slots + at);
      d[0] = make_uint4((uint32_t)h[j], (uint32_t)(h[j] >> 32), __float_as_uint(w[j]),
                        __float_as_uint(z));
      d[1] = make_uint4(__float_as_uint(n_seed), 0u, 0u, kSlotInit);
      c_new += fresh;
      c_over += !fresh;
      dnnz += fresh || w_old == 0.f;
    }
  }
  const int tot[kSeedCounts] = {wave_sum(c_new), wave_sum(c_over), wave_sum(c_foreign),
                                wave_sum(c_range), wave_sum(c_skip)};
  dnnz = wave_sum(dnnz);
  if ((threadIdx.x & 63) == 0) {
    unsigned long long* cs = counts + (int64_t)(blockIdx.x % count_stripes) * kAccStride;
#pragma unroll
    for (int c = 0; c < kSeedCounts; ++c)
      if (tot[c]) atomicAdd(&cs[c], (unsigned long long)tot[c]);
    if (stats && dnnz) atomicAdd(&acc_stripe(stats, acc_stripes)[0], (double)dnnz);
  }
}

// ---------------------------------------------------------------------------
// Host launchers
void kv_seed(const TableRef& t, KeyMix km, const uint64_t* raw, const float* w, int64_t n,
             uint64_t lo, uint64_t last, const UpdateParams& p, float n0,
             unsigned long long* counts, int count_stripes, const StripedAcc& stats,
             int32_t* err, hipStream_t st) {
  if (n <= 0) return;
  int lg = 0;
  while ((1ll << lg) < t.cap) ++lg;
  kv_seed_kernel<<<grid_for((n + kSeedBatch - 1) / kSeedBatch, 256), 256, 0, st>>>(
      (Slot*)t.slots, (uint64_t)(t.cap - 1), t.home_base, t.home_m, 64 - lg, km, raw, w, n, lo,
      last, p, n0, counts, count_stripes, stats.ptr, stats.stripes, err);
  PSAMD_HIP_CHECK(hipGetLastError());
}

void kv_rehash(const void* old_slots, int64_t old_cap, const TableRef& t,
               unsigned long long* moved, int stripes, int32_t* err, hipStream_t st) {
  int lg = 0;
  while ((1ll << lg) < t.cap) ++lg;
  kv_rehash_kernel<<<grid_for(old_cap, 256), 256, 0, st>>>(
      (const Slot*)old_slots, old_cap, (Slot*)t.slots, (uint64_t)(t.cap - 1), t.home_base,
      t.home_m, 64 - lg, moved, stripes, err);
  PSAMD_HIP_CHECK(hipGetLastError());
}

void kv_init(void* slots, int64_t cap, hipStream_t st) {
  kv_init_kernel<<<grid_for(cap, 256, 8192), 256, 0, st>>>((Slot*)slots, cap);
  PSAMD_HIP_CHECK(hipGetLastError());
}

void kv_resolve(const TableRef& t, const uint64_t* keys, int64_t n, const int32_t* n_dev,
                int64_t* out_slot, float* out_w, bool insert, const KeyInit& init, int32_t* err,
                int32_t* inserted, hipStream_t st) {
  int lg = 0;
  while ((1ll << lg) < t.cap) ++lg;
  kv_resolve_kernel<<<grid_for(n, 256), 256, 0, st>>>(
      (Slot*)t.slots, (uint64_t)(t.cap - 1), t.home_base, t.home_m, 64 - lg, keys, n, n_dev,
      out_slot, out_w, insert ? 1 : 0, init.type, init.v, init.s, init.seed, err, inserted);
  PSAMD_HIP_CHECK(hipGetLastError());
}

void kv_resolve_rows(const TableRef& t, const int32_t* recv, int G, int64_t H, int64_t C, int kw,
                     int64_t* out_slot, float* out_w, int64_t wstride, bool insert,
                     const KeyInit& init, int32_t* err, int32_t* inserted, uint64_t* out_key,
                     int32_t* bnd, int lgP, hipStream_t st) {
  int lg = 0;
  while ((1ll << lg) < t.cap) ++lg;
  dim3 grid(grid_for(C, 256, 1024), G);
  if (bnd && !t.home_m) throw std::runtime_error("kv_resolve_rows: partition bounds need an ordered home");
  kv_resolve_rows_kernel<<<grid, 256, 0, st>>>(
      (Slot*)t.slots, (uint64_t)(t.cap - 1), t.home_base, t.home_m, 64 - lg, recv, H, C, kw,
      out_slot, out_w, wstride > 0 ? wstride : C, insert ? 1 : 0, init.type, init.v, init.s,
      init.seed, err, inserted, out_key, bnd, lgP);
  PSAMD_HIP_CHECK(hipGetLastError());
}

void kv_gather(const void* slots, int64_t cap, const int64_t* slot_idx, int64_t n,
               const int32_t* n_dev, float* out, int field, hipStream_t st) {
  kv_gather_kernel<<<grid_for(n, 256), 256, 0, st>>>((const Slot*)slots, cap, slot_idx, n, n_dev,
                                                     out, field);
  PSAMD_HIP_CHECK(hipGetLastError());
}

void kv_set(void* slots, int64_t cap, const int64_t* slot_idx, int64_t n, const float* w,
            const float* z, const float* nn, hipStream_t st) {
  kv_set_kernel<<<grid_for(n, 256), 256, 0, st>>>((Slot*)slots, cap, slot_idx, n, w, z, nn);
  PSAMD_HIP_CHECK(hipGetLastError());
}

void kv_update(void* slots, int64_t cap, const int64_t* slot_idx, const float* grad, int64_t n,
               const int32_t* n_dev, const UpdateParams& p, const StripedAcc& stats,
               const AucOut& auc, hipStream_t st) {
  if (auc.hist && auc.nbins != 2048)
    throw std::runtime_error("kv_update: the fused AUC needs 2048 bins");
  kv_update_kernel<<<grid_for(n, 256), 256, 0, st>>>(
      (Slot*)slots, cap, slot_idx, grad, n, n_dev, p, stats.ptr, stats.stripes, auc.hist,
      auc.nbins, auc.stripes, auc.metrics, auc.step_counter);
  PSAMD_HIP_CHECK(hipGetLastError());
}

void kv_accumulate(void* slots, int64_t cap, const int64_t* slot_idx, const float* grad,
                   int64_t n, const int32_t* n_dev, int64_t* touched, int32_t* n_touched,
                   int64_t touched_cap, hipStream_t st) {
  kv_accumulate_kernel<<<grid_for(n, 256), 256, 0, st>>>((Slot*)slots, cap, slot_idx, grad, n,
                                                         n_dev, touched, n_touched, touched_cap);
  PSAMD_HIP_CHECK(hipGetLastError());
}

void kv_accumulate_rows(void* slots, int64_t cap, const int64_t* slot_idx, const float* grad,
                        int64_t gstride, const int32_t* recv, int G, int64_t H, int64_t C,
                        int64_t* touched, int32_t* n_touched, int64_t touched_cap,
                        hipStream_t st) {
  dim3 grid(grid_for(C, 256, 1024), G);
  kv_accumulate_rows_kernel<<<grid, 256, 0, st>>>((Slot*)slots, cap, slot_idx, grad, gstride, recv,
                                                  H, C, touched, n_touched, touched_cap);
  PSAMD_HIP_CHECK(hipGetLastError());
}

void kv_apply_accumulated(void* slots, int64_t cap, const int64_t* touched,
                          const int32_t* n_touched, int64_t max_n, const UpdateParams& p,
                          const StripedAcc& stats, hipStream_t st) {
  kv_apply_accumulated_kernel<<<grid_for(max_n, 256), 256, 0, st>>>(
      (Slot*)slots, cap, touched, n_touched, max_n, p, stats.ptr, stats.stripes);
  PSAMD_HIP_CHECK(hipGetLastError());
}

void kv_update_rows(void* slots, int64_t cap, const int64_t* slot_idx, const float* grad,
                    int64_t gstride, const int32_t* recv, int G, int64_t H, int64_t C,
                    unsigned long long* link, int64_t link_size, int32_t* nxt,
                    const UpdateParams& p, const StripedAcc& stats, hipStream_t st) {
  if (cap > (int64_t(1) << 32)) throw std::runtime_error("kv_update_rows: capacity > 2^32");
  if (link_size < 2 * (int64_t)G * C || (link_size & (link_size - 1)))
    throw std::runtime_error("kv_update_rows: link scratch must be a power of two >= 2*G*C");
  if (G < 1 || G > kMaxChain) throw std::runtime_error("kv_update_rows: 1..64 source rows");
  fill_async<unsigned long long>(link, link_size, ~0ull, st);
  dim3 grid(grid_for(C, 256, 1024), G);
  kv_link_rows_kernel<<<grid, 256, 0, st>>>(slot_idx, cap, grad, gstride, recv, H, C, link,
                                            (uint64_t)(link_size - 1), nxt);
  PSAMD_HIP_CHECK(hipGetLastError());
  kv_apply_rows_kernel<<<grid, 256, 0, st>>>((Slot*)slots, cap, slot_idx, grad, gstride, recv, H,
                                             C, link, (uint64_t)(link_size - 1), nxt,
                                             (int64_t)G * C, p, stats.ptr, stats.stripes);
  PSAMD_HIP_CHECK(hipGetLastError());
}

void kv_apply_part(void* slots, int64_t cap, const int64_t* slot_idx, const uint64_t* keys,
                   const float* grad, int64_t gstride, const int32_t* recv, int G, int64_t H,
                   int64_t C, const int32_t* bnd, int lgP, const UpdateParams& p,
                   const StripedAcc& stats, int ffnb, int kw, hipStream_t st) {
  if (cap > (int64_t(1) << 32) - 1) throw std::runtime_error("kv_apply_part: capacity >= 2^32");
  if ((int64_t)G * C >= (int64_t(1) << 31)) throw std::runtime_error("kv_apply_part: G*C >= 2^31");
  if (G < 1 || G > kMaxChain) throw std::runtime_error("kv_apply_part: 1..64 source rows");
  if (lgP < 0 || lgP > 20) throw std::runtime_error("kv_apply_part: lgP in 0..20");
  kv_apply_part_kernel<<<1 << lgP, 256, 0, st>>>((Slot*)slots, cap, slot_idx, keys, grad, gstride,
                                                 recv, H, C, G, bnd, lgP, p, stats.ptr,
                                                 stats.stripes, ffnb, kw);
  PSAMD_HIP_CHECK(hipGetLastError());
}

void kv_census(const void* slots, int64_t cap, unsigned long long* out, hipStream_t st) {
  kv_census_kernel<<<grid_for(cap, 256, 4096), 256, 0, st>>>((const Slot*)slots, cap, out);
  PSAMD_HIP_CHECK(hipGetLastError());
}

}  // namespace psamd
