// Device side shared by the units of the "tp" / "tpf" kernel family (tploc.hip,
// tploc_bucket.hip, tploc_flat.hip, tploc_fused.hip, tploc_step.hip): the tile / bucket
// geometry constants, the workgroup scan and hash helpers, the LDS build and rank sort of
// the two bucket kernels (tploc_bucket.hip), the 64-bit fixed-point accumulation of every
// backward in the family, and the flat layout's regions and block -> group map. Helpers only: every kernel, and every __device__ variable, lives in
// the unit that launches it.
#pragma once
#include "tploc.h"

namespace psamd {

namespace tp {
constexpr int kThr = 1024;              // tile workgroup
// 8192 occurrences per tile (a 65,536 x 39 minibatch is 313 tiles). Measured and not
// kept: 10,240 (250 tiles, at most one per CU): tile 24.7 -> 24.2 us and fused
// forward+backward 24.3 -> 23.7, but 136 / 87 KB of LDS per workgroup left no room for
// the other streams' kernels and the pipelined step went 0.118 -> 0.126 ms
// (profiles/r3_tile_count.log).
constexpr int kIt = 8;
constexpr int kTile = kThr * kIt;       // 8192 occurrences
constexpr int kHash = 2 * kTile;        // LDS hash slots of a tile (load <= 0.5)
constexpr int kHB = 14;                 // log2 kHash
// Quotient encoding of the tile hash: a key k (<= 34 bits, uniformly mixed) probes from
// home slot k mod kHash, and the slot keeps (k >> kHB) << kDispB | displacement, which
// with the slot index gives k back: 34-bit keys in 32-bit LDS words.
constexpr int kDispB = 12;
constexpr uint32_t kMaxDisp = (1u << kDispB) - 1;  // never reached at load <= 0.5
constexpr int kMaxBk = 2048;            // buckets (tile LDS: 72 KB -> 2 workgroups per CU)
constexpr int kMaxT = 640;              // tiles (n <= 5.2 M)
constexpr int kBThr = 256;              // emit workgroups
constexpr int kBkThr = 512;             // bucket workgroups
constexpr int kECap = 4096;             // entries of one bucket (global stride)
constexpr int kECapL = 4064;            // ... held in LDS (bucket kernel LDS <= 40 KB:
                                        // 4 workgroups per CU instead of 3)
constexpr int kDH = 2048;               // distinct-key hash of one bucket
constexpr int kBkProbe = 128;           // probe chain bound of the bucket hash build
constexpr uint32_t kEmpty = 0xffffffffu;
constexpr int kG = (kECapL + kBkThr - 1) / kBkThr;  // entries per thread
}  // namespace tp

__device__ __forceinline__ uint32_t tp_hash(uint32_t x) {
  x ^= x >> 16;
  x *= 0x7feb352du;
  x ^= x >> 15;
  x *= 0x846ca68bu;
  x ^= x >> 16;
  return x;
}

template <int kN>
__device__ __forceinline__ uint32_t tp_block_scan(uint32_t v, uint32_t* lds, uint32_t* total) {
  constexpr int kW = kN / 64;
  const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
  uint32_t x = v;
#pragma unroll
  for (int off = 1; off < 64; off <<= 1) {
    const uint32_t y = __shfl_up(x, off, 64);
    if (lane >= off) x += y;
  }
  if (lane == 63) lds[wid] = x;
  __syncthreads();
  if (threadIdx.x == 0) {
    uint32_t run = 0;
    for (int w = 0; w < kW; ++w) {
      const uint32_t t = lds[w];
      lds[w] = run;
      run += t;
    }
    lds[kW] = run;
  }
  __syncthreads();
  const uint32_t r = x - v + lds[wid];
  *total = lds[kW];
  __syncthreads();
  return r;
}

// sum of a[0:b) by one workgroup (a few thousand L2-resident words)
template <int kN>
__device__ __forceinline__ uint32_t tp_prefix(const uint32_t* __restrict__ a, int b, uint32_t* lds) {
  uint32_t s = 0;
  for (int i = threadIdx.x; i < b; i += kN) s += a[i];
  uint32_t tot;
  tp_block_scan<kN>(s, lds, &tot);
  return tot;
}

__device__ __forceinline__ uint64_t tp_match_any(uint32_t v, int nbits, uint64_t active) {
  uint64_t peers = active;
  for (int b = 0; b < nbits; ++b) {
    const bool bit = (v >> b) & 1u;
    const uint64_t bal = __ballot(bit);
    peers &= bit ? bal : ~bal;
  }
  return peers;
}

// ------------------------------------------- bucket build + rank sort (both layouts)
// Build the dedup state of fine buckets [f0, f0 + nf) (nf = 2: a pair; the key inserted
// is (hb + fine bucket - f0) << shift | suffix). Leaves: eh[g] = hash slot of entry g,
// idx[] = tile entry ids (registers), hkey / hcnt = the hash, dl[0..D) = the compacted
// occupied slots. Returns (block-uniform) whether every entry found a slot within the
// LDS capacity; *E / *D = entries / distinct keys.
template <bool kCnt = false>  // kCnt: hcnt sums the entries' occurrence counts (ecnt)
__device__ __forceinline__ bool tp_bk_build(const uint32_t* __restrict__ tkeys,
                                            const uint16_t* __restrict__ toff, int nbf, int T,
                                            int shift, int f0, int nf, uint32_t hb,
                                            uint32_t* hkey, uint32_t* hcnt, uint64_t* dl,
                                            uint16_t* eh, uint32_t* lds, uint32_t* flag,
                                            int32_t (&idx)[tp::kG], uint32_t* E_out,
                                            uint32_t* D_out, uint64_t* prof,
                                            const uint8_t* __restrict__ ecnt = nullptr) {
  using namespace tp;
  const int t = threadIdx.x;
  uint32_t* tpre = reinterpret_cast<uint32_t*>(dl);                // [kMaxT + 1]
  uint16_t* tlo = reinterpret_cast<uint16_t*>(tpre + kMaxT + 1);  // [kMaxT]
  uint16_t* tmid = tlo + kMaxT;                                   // [kMaxT]
  for (int s = t; s < kDH; s += kBkThr) {
    hkey[s] = kEmpty;
    hcnt[s] = 0;
  }
  if (t == 0) *flag = 0;
  // per-tile runs [toff[q][f0], toff[q][f0 + nf]): thread t owns tiles [t*per, t*per + per)
  const int per = (T + kBkThr - 1) / kBkThr;
  const int q0 = t * per, q1 = q0 + per < T ? q0 + per : T;
  uint32_t c = 0;
  for (int q = q0; q < q1; ++q) {
    const uint16_t* to = toff + (int64_t)q * (nbf + 1);
    const uint32_t lo = to[f0], hi = to[f0 + nf];
    tlo[q] = (uint16_t)lo;
    tmid[q] = (uint16_t)((nf == 2 ? to[f0 + 1] : hi) - lo);
    tpre[q] = hi - lo;
    c += hi - lo;
  }
  uint32_t E;
  uint32_t w = tp_block_scan<kBkThr>(c, lds, &E);
  for (int q = q0; q < q1; ++q) {
    const uint32_t len = tpre[q];
    tpre[q] = w;
    w += len;
  }
  if (t == 0) tpre[T] = E;
  __syncthreads();
  if (prof && t == 0) prof[(int64_t)blockIdx.x * 12 + 1] = clock64();
  const uint32_t En = E < (uint32_t)kECapL ? E : (uint32_t)kECapL;
  bool bad = E > (uint32_t)kECapL;
  uint32_t hib = 0;  // bit q: entry q lies in the pair's second fine bucket
#pragma unroll
  for (int q = 0; q < kG; ++q) {
    const uint32_t g = q * kBkThr + t;
    idx[q] = -1;
    if (g < En) {
      int lo = 0, up = T - 1;  // last tile with tpre[q] <= g
      while (lo < up) {
        const int mid = (lo + up + 1) >> 1;
        if (tpre[mid] <= g) lo = mid; else up = mid - 1;
      }
      const uint32_t off = g - tpre[lo];
      idx[q] = lo * kTile + tlo[lo] + (int32_t)off;
      hib |= (off >= tmid[lo] ? 1u : 0u) << q;
    }
  }
  uint32_t kv[kG];
  uint32_t ecp[(kG + 3) / 4];  // (kCnt: the entries' occurrence counts, 4 bytes a word)
#pragma unroll
  for (int q = 0; q < kG; ++q) kv[q] = idx[q] >= 0 ? tkeys[idx[q]] : 0u;
  if (kCnt) {
#pragma unroll
    for (int w = 0; w < (kG + 3) / 4; ++w) ecp[w] = 0u;
#pragma unroll
    for (int q = 0; q < kG; ++q)
      if (idx[q] >= 0) ecp[q >> 2] |= (uint32_t)ecnt[idx[q]] << ((q & 3) * 8);
  }
#pragma unroll
  for (int q = 0; q < kG; ++q) {
    if (idx[q] < 0) continue;
    const uint32_t g = q * kBkThr + t;
    const uint32_t key = kv[q] | ((hb + ((hib >> q) & 1u)) << shift);
    uint32_t h = tp_hash(key) & (kDH - 1);
    bool ok = false;
    // (another lane gave up: the build is lost anyway)
    bad |= __hip_atomic_load(flag, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP) != 0u;
    // (bounded chain: a hash this full -- near-distinct keys -- is cheaper to give up on
    // than to probe through: the overflow form takes the pair, profiles/r6_skew_layout.log)
    for (int p = 0; p < kBkProbe && !bad; ++p) {
      const uint32_t cu = hkey[h];
      if (cu == kEmpty) {
        const uint32_t prev = atomicCAS(&hkey[h], kEmpty, key);
        if (prev == kEmpty || prev == key) { ok = true; break; }
      } else if (cu == key) {
        ok = true;
        break;
      }
      h = (h + 1) & (kDH - 1);
    }
    if (ok) {
      atomicAdd(&hcnt[h], kCnt ? (ecp[q >> 2] >> ((q & 3) * 8)) & 0xffu : 1u);
    } else if (!bad) {
      bad = true;
      atomicOr(flag, 1u);
    }
    eh[g] = ok ? (uint16_t)h : (uint16_t)0xffffu;
  }
  if (bad) atomicOr(flag, 1u);
  __syncthreads();
  if (prof && t == 0) prof[(int64_t)blockIdx.x * 12 + 2] = clock64();
  // compact the occupied slots (strided: conflict-free LDS reads)
  constexpr int kPer = kDH / kBkThr;  // 4
  uint64_t ent[kPer];
  uint32_t cc = 0;
#pragma unroll
  for (int q = 0; q < kPer; ++q) {
    const int s = q * kBkThr + t;
    ent[q] = hkey[s] != kEmpty
                 ? (((uint64_t)hkey[s] << 32) |
                    ((uint64_t)(kCnt ? min(hcnt[s], 0xffffu) : hcnt[s]) << 16) | (uint64_t)s)
                 : ~0ull;
    cc += ent[q] != ~0ull;
  }
  uint32_t D;
  uint32_t wd = tp_block_scan<kBkThr>(cc, lds, &D);  // (its barriers: every locate is done)
#pragma unroll
  for (int q = 0; q < kPer; ++q)
    if (ent[q] != ~0ull) dl[wd++] = ent[q];
  *E_out = En;
  *D_out = D;
  const bool good = *flag == 0u;
  __syncthreads();
  return good;
}

// rank sort of dl[0..D) into hs (distinct keys: rank = # smaller keys). Broadcast LDS
// reads, two keys per 16-B read and four reads in flight; dl[D .. D+7] padded with ~0
// (larger than any entry: key < 2^32 in the high word) so the tail needs no test. With
// <= 256 keys, 2 or 4 threads split each key's scan and add their counts in LDS.
__device__ __forceinline__ void tp_bk_ranksort(uint64_t* dl, uint64_t* hs, uint32_t D) {
  using namespace tp;
  const int t = threadIdx.x;
  if (t < 8 && D + t < (uint32_t)kDH) dl[D + t] = ~0ull;
  uint32_t* rk = reinterpret_cast<uint32_t*>(hs + 1024);  // beyond any output rank < 256
  const int tpk = D <= 128 ? 4 : D <= 256 ? 2 : 1;
  if (tpk > 1 && t < 256) rk[t] = 0;
  __syncthreads();
  const uint4* d4 = reinterpret_cast<const uint4*>(dl);
  const uint32_t nq = (D + 7) / 8;
  if (tpk > 1) {
    const int nk = kBkThr / tpk, i = t % nk, h = t / nk;
    const uint32_t pq = (nq + tpk - 1) / tpk;
    const uint32_t qa = h * pq, qb = qa + pq < nq ? qa + pq : nq;
    if ((uint32_t)i < D) {
      const uint64_t x = dl[i];
      uint32_t r = 0;
      for (uint32_t q = qa; q < qb; ++q) {
        uint4 v[4];
#pragma unroll
        for (int k = 0; k < 4; ++k) v[k] = d4[q * 4 + k];
#pragma unroll
        for (int k = 0; k < 4; ++k) {
          r += (((uint64_t)v[k].y << 32) | v[k].x) < x;
          r += (((uint64_t)v[k].w << 32) | v[k].z) < x;
        }
      }
      atomicAdd(&rk[i], r);
    }
    __syncthreads();
    if (h == 0 && (uint32_t)i < D) hs[rk[i]] = dl[i];
  } else {
    for (uint32_t i = t; i < D; i += kBkThr) {
      const uint64_t x = dl[i];
      uint32_t r = 0;
      for (uint32_t q = 0; q < nq; ++q) {
        uint4 v[4];
#pragma unroll
        for (int k = 0; k < 4; ++k) v[k] = d4[q * 4 + k];
#pragma unroll
        for (int k = 0; k < 4; ++k) {
          r += (((uint64_t)v[k].y << 32) | v[k].x) < x;
          r += (((uint64_t)v[k].w << 32) | v[k].z) < x;
        }
      }
      hs[r] = x;
    }
  }
}

// -------------------------------------------------------------------- backward
// psum[tile entry] = sum over the tile's occurrences of the entry of coef[row] * val.
// Tiles accumulate in 64-bit FIXED POINT with integer LDS atomics (gfx950: ds_add_f32
// ~195 cycles per wave-instruction, ds_add_u64 ~13-18; profiles/r2_lds_atomics.log):
// scale 2^(48 - e) with every |addend| < 2^e keeps any sum of a tile's 8192 addends
// below 2^61, and the partials are exactly rounded, order-independent sums.
__device__ __forceinline__ int fx_shift(uint32_t maxbits) {
  int e = 0;
  if (maxbits) (void)frexpf(__uint_as_float(maxbits), &e);
  return min(100, 48 - e);
}
__device__ __forceinline__ void fx_add(long long* acc, int idx, float v, double sc) {
  const long long fx = __double2ll_rn((double)v * sc);
  if (fx) atomicAdd(reinterpret_cast<unsigned long long*>(&acc[idx]), (unsigned long long)fx);
}
// every wave's max |v| -> the tile's (LDS ds_max_u32 on the float bits of |v|)
__device__ __forceinline__ void fx_tile_max(float vmax, uint32_t* smax) {
  vmax = wave_max(vmax);
  if ((threadIdx.x & 63) == 0 && vmax > 0.f) atomicMax(smax, __float_as_uint(vmax));
}

// ====================================================================== flat ("tpf")
// The 1-GPU layout: the bucket stage writes FIXED per-workgroup output regions instead of
// one compact sorted array, so no bucket waits for another (the compact layout's
// decoupled look-back: 11 k of 47 k cycles per workgroup, r3_tp_pair_phases.log) and
// nothing is rank-sorted or laid out as a CSC. Bucket workgroup b (a pair of fine
// buckets, the tp_bucket geometry) owns
//   keys     uniqf[b * kUC + s * kUnitK + j], j < D_s   (unit s = 0; units 0 and 1 when an
//            overflowing pair falls back to its two fine buckets one after the other)
//   entries  ent_pos / ent_j[b * kEC + e]: tile entry id (tile * 8192 + e) and the unit's
//            key index j of every tile-distinct entry of the unit's keys (unit 1 after
//            the E_0 entries of unit 0)
//   counts   cnt[b * 4 + {D_0, E_0, D_1, E_1}]
// The consumers run one workgroup per bucket workgroup and combine in LDS: tpf_step sums
// each key's entry partials (fixed point) and applies the update, then pulls the next
// minibatch's keys and scatters their weights into its tile-entry order (w_ent), which
// the fused forward reads contiguously. Keys of one key-range bucket stay in the same
// bucket workgroup for every minibatch of the same size, so a key's update and its next
// pull run in the same workgroup, in that order.
namespace tpf {
constexpr int kUnitK = tp::kDH;  // keys of one unit (the bucket hash)
constexpr int kUC = 2 * kUnitK;  // key region of a bucket workgroup (two units)
constexpr int kEC = 8192;        // entry region of a bucket workgroup
constexpr int kThr = 256;        // tpf_step workgroup (auc_hist_block: an extra last one)
constexpr uint32_t kNoSlot = 0xffffffffu;
}  // namespace tpf

// Physical block index -> logical bucket group of the flat bucket-geometry kernels.
// Entries are laid out per tile (tkeys / psum / w_ent / ecnt[tile * 8192 + position],
// position = the tile's counting-sort order by fine bucket), so a group's run inside one
// tile is a few entries and one 128-B line of those arrays (and of a tile's toff row)
// holds the runs of ~10 (32) neighbouring groups. Blocks are dealt round-robin over the 8
// XCDs, each with a private L2: with b = blockIdx.x neighbouring groups sit on 8 different
// XCDs and every such line is fetched into (or partially written from) all 8 L2s. This
// bijective remap (the form of gemm.hip xcd_swizzle) gives the blocks of one XCD
// (bid % 8) a contiguous range of groups. The identity for groups < 8. `groups` is the
// bucket groups, never gridDim.x: tpf_step / tpf_pack_grads launch one extra block (AUC /
// overflow), which stays the last physical block and is not remapped. Every kernel that
// uses it is a pure function of its group (no group waits for another); acc_stripe, the
// hist stripes and the prof slots only spread contention and stay on blockIdx.x.
// Used by tpf_step_kernel, tpf_unpack_w_kernel and tpf_pack_grads_kernel (device-only,
// 65,536 x 39, 1024 groups, benchmarks/micro/tpf_xcd_probe.py: step 23.6 -> 18.3 us with
// L2 fabric reads 802 k -> 593 k and writes 702 k -> 400 k per launch, unpack_w 8.8 -> 5.6,
// pack_grads 8.9 -> 6.6; profiles/xcd_remap.log). Measured and not kept (a kernel keeps
// the map only where its own probe time improves by more than its repeats' spread):
//   tpf_bucket_kernel   fabric reads 320 k -> 47 k per launch, but 16.3 -> 16.4-16.6 us
//                       (bound by its LDS build, not by these misses); with it mapped too
//                       the 300-step headline read 0.0743-0.0751 vs 0.0752-0.0754 ms
//   tpf_filter_kernel   17.4-18.8 min / 34.9-37.0 median vs 18.0-18.3 / 36.1-37.9 us in
//                       the tail-filtered pipeline: no difference
//   tpf_pack_keys_kernel  3.24 vs 3.20 us: it reads its keys contiguously per group
// NOT for tp_bucket_kernel (compact layout): its decoupled look-back relies on dispatch
// in blockIdx order (a bucket only waits for buckets that are running or done); remapped,
// a block could spin on one that is not yet resident. Not for the tile-partitioned kernels
// either (tp_tile, tp_fwd_bwd*): their blocks share no lines.
__host__ __device__ __forceinline__ int tpf_xcd_group_of(int bid, int groups) {
  if (groups < 8) return bid;
  const int q = groups >> 3, r = groups & 7, xcd = bid & 7;
  const int base = xcd < r ? xcd * (q + 1) : r * (q + 1) + (xcd - r) * q;
  return base + (bid >> 3);
}

}  // namespace psamd
