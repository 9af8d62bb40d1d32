// The bucket stage of the "tp" localisation (tile stage: tploc.hip), for both layouts:
//   tp_bucket_kernel    compact layout: sorted unique keys, entry CSC and ent_uid, the
//                       buckets' global bases by a decoupled look-back (localize_tp)
//   tpf_bucket_kernel   flat 1-GPU layout: fixed per-workgroup regions, no look-back,
//                       no CSC (tpf_launch_bucket, called by tploc_flat.hip localize_tpf)
// Both gather a pair of fine buckets with the LDS build of tploc.cuh (tp_bk_build); a pair
// that overflows it falls back to its fine buckets one after the other, register-light
// (tp_bk_fine_light / tpf_unit_light). The three routines look alike and stay apart: each
// one's register budget was tuned on its own. The two kernels share one unit because both
// inline tp_bk_build<false>: compiled in separate units, each came out with a different
// register assignment than compiled together (same resource usage, a few instructions
// apart), and their tuning was measured on the code they have together
// (profiles/tploc_split.md).
#include "tploc.cuh"
#include "tploc_geom.h"

#include <stdexcept>

namespace psamd {

// ---------------------------------------------------------------------- bucket
// One workgroup per COARSE bucket c: the fine buckets 2c and 2c+1 of the tile kernel's
// counting sort (a range of the mixed key space; the two runs of a tile are adjacent,
// so the pair is one run per tile). It dedups the pair AND writes its slice of the
// global outputs:
//   build          the entries from every tile (flat: each thread locates its entries
//                  by binary search over the per-tile run prefix and loads them
//                  together; the entry ids stay in registers), each key (suffix plus the
//                  fine bucket's low bit above it) inserted into an LDS hash with an entry
//                  count, then the occupied slots compacted -> (key | count | slot) list;
//                  the pair's distinct and entry counts are PUBLISHED for the look-back
//   rank sort      distinct keys are unique: rank = number of smaller keys (2 or 4
//                  threads per key when they are few)
//   look-back      one wave derives the bucket's global bases (unique ids, entries) from
//                  the earlier buckets' published counts (decoupled look-back: 64 status
//                  words per step, nearest inclusive prefix ends it) and publishes its
//                  own inclusive prefix
//   starts         prefix of the counts in key order -> uniq, seg_start (global)
//   assign         every entry takes the next position of its key's segment (LDS
//                  atomic: the order inside a segment is not fixed) -> entry CSC
//                  (pos_s, segid), ent_uid
// Pairs: 1024 workgroups of 512 threads at 40 KB of LDS are ONE round on the 256 CUs
// (2048 single buckets were two rounds, 43 us; profiles/r3_tp_phases.log). A pair whose
// entries overflow the LDS capacity (or its hash) falls back to its two fine buckets one
// after the other: count both, publish, look back, then build / sort / write each again.
// The fine geometry (<= 1280 occurrences per fine bucket) keeps that fallback exact even
// when every key is distinct.
// Workgroups are dispatched in blockIdx order, so a bucket only ever waits for buckets
// that are running or done; the spin is bounded anyway (err bit 4, no hang). The status
// words carry an 8-bit launch epoch (device counter, advanced by the last bucket), so
// they need no reset between launches or graph replays.
// Per-phase shader-clock marks (prof != null) are a tuning aid
// (benchmarks/prof_tp_phases.py).
namespace tp {
constexpr uint64_t kStA = 1, kStP = 2;  // status flags: aggregate / inclusive prefix
constexpr uint32_t kStM = (1u << 27) - 1;
}  // namespace tp
__device__ __forceinline__ uint64_t tp_status(uint32_t ep, uint64_t flag, uint32_t d, uint32_t e) {
  return ((uint64_t)ep << 56) | (flag << 54) | ((uint64_t)(d & tp::kStM) << 27) | (e & tp::kStM);
}

// starts + assign: the sorted keys hs[0..D) -> uniq / seg_start from (ubase, ebase);
// every entry of idx[] takes the next position of its key's segment.
__device__ __forceinline__ void tp_bk_emit(const uint64_t* hs, uint64_t* dl, const uint16_t* eh,
                                           const int32_t (&idx)[tp::kG], uint32_t D,
                                           uint32_t ubase, uint32_t ebase, uint64_t key0,
                                           uint32_t* lds, int32_t* __restrict__ pos_s,
                                           int32_t* __restrict__ segid,
                                           uint64_t* __restrict__ uniq,
                                           int32_t* __restrict__ seg_start,
                                           int32_t* __restrict__ ent_uid,
                                           float* __restrict__ zero_a,
                                           unsigned long long* __restrict__ zero_b,
                                           int64_t u_cap, int64_t e_cap, uint64_t* prof) {
  using namespace tp;
  const int t = threadIdx.x;
  uint32_t* cur = reinterpret_cast<uint32_t*>(dl);        // [kDH] per slot
  uint16_t* jj = reinterpret_cast<uint16_t*>(cur + kDH);  // [kDH] per slot
  __syncthreads();  // (dl: the rank sort's source is dead)
  uint32_t carry = 0;
  for (uint32_t j0 = 0; j0 < D; j0 += kBkThr) {
    const uint32_t j = j0 + t;
    const uint64_t v = j < D ? hs[j] : 0ull;
    const uint32_t cnt = (uint32_t)(v >> 16) & 0xffffu;
    uint32_t tot;
    const uint32_t ex = tp_block_scan<kBkThr>(cnt, lds, &tot) + carry;
    if (j < D) {
      const uint32_t slot = (uint32_t)v & 0xffffu;
      const int64_t u = (int64_t)ubase + j;
      if (in_range(u, u_cap)) {
        uniq[u] = key0 | (uint32_t)(v >> 32);
        seg_start[u] = (int32_t)(ebase + ex);
        if (zero_a) zero_a[u] = 0.f;
        if (zero_b) zero_b[u] = 0ull;
      }
      cur[slot] = ex;
      jj[slot] = (uint16_t)j;
    }
    carry += tot;
  }
  __syncthreads();
  if (prof && t == 0) prof[(int64_t)blockIdx.x * 12 + 6] = clock64();
#pragma unroll
  for (int q = 0; q < kG; ++q) {
    if (idx[q] < 0) continue;
    const uint32_t h = eh[q * kBkThr + t];
    if (h == 0xffffu) continue;
    const uint32_t pos = atomicAdd(&cur[h], 1u);
    const uint32_t u = ubase + jj[h];
    const int64_t e = (int64_t)ebase + pos;
    if (in_range(e, e_cap)) {
      pos_s[e] = idx[q];
      segid[e] = (int32_t)(u + 1);
    }
    if (in_range((int64_t)idx[q], e_cap)) ent_uid[idx[q]] = (int32_t)u;
  }
  __syncthreads();
}

// Decoupled look-back of fine bucket fs (wave 0; the caller syncs after): the bases
// (sums of every earlier fine bucket's counts) go to sb[1] / sb[2]; the inclusive prefix
// is published at fs and at twin (a pair's second fine bucket, published empty); the
// workgroup holding the last fine bucket writes the totals and advances the epoch.
__device__ __forceinline__ void tp_bk_lookback(uint64_t* __restrict__ status, int fs, int twin,
                                               int nbf, uint32_t ep, uint32_t D, uint32_t E,
                                               uint32_t* sb, uint32_t* __restrict__ epoch,
                                               int32_t* __restrict__ n_uniq,
                                               int32_t* __restrict__ n_ent,
                                               int32_t* __restrict__ seg_start, int64_t u_cap,
                                               int32_t* __restrict__ err) {
  using namespace tp;
  const int lane = threadIdx.x;
  if (lane >= 64) return;
  uint32_t su = 0, se = 0;
  if (fs > 0) {
    int j = fs - 1;
    uint32_t spins = 0;
    while (true) {
      const int jl = j - lane;  // lane 0 = nearest earlier bucket
      const uint64_t st =
          jl >= 0 ? __hip_atomic_load(&status[jl], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)
                  : tp_status(ep, kStP, 0, 0);
      const uint32_t f = (uint32_t)(st >> 56) == ep ? (uint32_t)(st >> 54) & 3u : 0u;
      const uint64_t pm = __ballot(f == kStP), nr = __ballot(f == 0);
      const int fp = pm ? __builtin_ctzll(pm) : 64;  // nearest inclusive prefix
      const uint64_t need = fp >= 63 ? ~0ull : ((2ull << fp) - 1);
      if (nr & need) {  // an earlier bucket has not published yet
        if (++spins > (1u << 22)) {
          if (lane == 0) atomicOr(err, 4);
          break;
        }
        __builtin_amdgcn_s_sleep(1);
        continue;
      }
      const bool inc = lane <= fp;
      su += wave_allsum(inc ? (uint32_t)(st >> 27) & kStM : 0u);
      se += wave_allsum(inc ? (uint32_t)st & kStM : 0u);
      if (fp < 64) break;
      j -= 64;
    }
  }
  if (lane == 0) {
    const uint64_t inc = tp_status(ep, kStP, su + D, se + E);
    if (fs > 0) __hip_atomic_store(&status[fs], inc, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    if (twin != fs) __hip_atomic_store(&status[twin], inc, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    sb[1] = su;
    sb[2] = se;
    if (twin == nbf - 1) {  // every bucket has published: the launch is done with the epoch
      const uint32_t U = su + D, Et = se + E;
      *n_uniq = (int32_t)U;
      *n_ent = (int32_t)Et;
      if (in_range((int64_t)U, u_cap + 1)) seg_start[U] = (int32_t)Et;
      __hip_atomic_store(epoch, ep, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
  }
}

// Fallback for one fine bucket f of an overflowing pair, register-light (plain loops,
// no per-thread entry arrays, so it does not raise the common path's register count):
// the per-tile runs live in the eh region, entries are located again for the assign
// and find their key's rank by binary search in the sorted list.
__device__ __forceinline__ void tp_bk_fine_light(
    const uint32_t* __restrict__ tkeys, const uint16_t* __restrict__ toff, int nbf, int T,
    int shift, int f, uint32_t hb, uint64_t key0, uint32_t* hkey, uint32_t* hcnt, uint64_t* hs,
    uint64_t* dl, uint16_t* ehraw, uint32_t* lds, uint32_t* sb, uint64_t* __restrict__ status,
    uint32_t ep, uint32_t* __restrict__ epoch, int32_t* __restrict__ pos_s,
    int32_t* __restrict__ segid, uint64_t* __restrict__ uniq, int32_t* __restrict__ seg_start,
    int32_t* __restrict__ ent_uid, int32_t* __restrict__ n_uniq, int32_t* __restrict__ n_ent,
    float* __restrict__ zero_a, unsigned long long* __restrict__ zero_b, int64_t u_cap,
    int64_t e_cap, int32_t* __restrict__ err) {
  using namespace tp;
  static_assert((kMaxT + 1) * 4 + kMaxT * 2 <= kECapL * 2, "tile runs must fit in eh");
  const int t = threadIdx.x;
  uint32_t* tpre = reinterpret_cast<uint32_t*>(ehraw);             // [kMaxT + 1]
  uint16_t* tlo = reinterpret_cast<uint16_t*>(tpre + kMaxT + 1);  // [kMaxT]
  for (int s = t; s < kDH; s += kBkThr) {
    hkey[s] = kEmpty;
    hcnt[s] = 0;
  }
  const int per = (T + kBkThr - 1) / kBkThr;
  const int q0 = t * per, q1 = q0 + per < T ? q0 + per : T;
  uint32_t c = 0;
  for (int q = q0; q < q1; ++q) {
    const uint16_t* to = toff + (int64_t)q * (nbf + 1);
    const uint32_t lo = to[f], hi = to[f + 1];
    tlo[q] = (uint16_t)lo;
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
  auto locate = [&](uint32_t g) -> int32_t {
    int lo = 0, up = T - 1;  // last tile with tpre[q] <= g
    while (lo < up) {
      const int mid = (lo + up + 1) >> 1;
      if (tpre[mid] <= g) lo = mid; else up = mid - 1;
    }
    return lo * kTile + tlo[lo] + (int32_t)(g - tpre[lo]);
  };
  bool bad = false;
  for (uint32_t g = t; g < E; g += kBkThr) {
    const uint32_t key = tkeys[locate(g)] | (hb << shift);
    uint32_t h = tp_hash(key) & (kDH - 1);
    bool ok = false;
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
    if (ok) atomicAdd(&hcnt[h], 1u);
    else bad = true;
  }
  if (bad) atomicOr(err, 1);
  __syncthreads();
  constexpr int kPer = kDH / kBkThr;
  uint32_t cc = 0;
  for (int q = 0; q < kPer; ++q) cc += hkey[q * kBkThr + t] != kEmpty;
  uint32_t D;
  uint32_t wd = tp_block_scan<kBkThr>(cc, lds, &D);
  for (int q = 0; q < kPer; ++q) {
    const int s = q * kBkThr + t;
    if (hkey[s] != kEmpty) dl[wd++] = ((uint64_t)hkey[s] << 32) | ((uint64_t)hcnt[s] << 16) | (uint64_t)s;
  }
  if (t == 0)
    __hip_atomic_store(&status[f], tp_status(ep, f == 0 ? kStP : kStA, D, E), __ATOMIC_RELAXED,
                       __HIP_MEMORY_SCOPE_AGENT);
  __syncthreads();
  tp_bk_ranksort(dl, hs, D);
  tp_bk_lookback(status, f, f, nbf, ep, D, E, sb, epoch, n_uniq, n_ent, seg_start, u_cap, err);
  __syncthreads();
  const uint32_t ubase = sb[1], ebase = sb[2];
  uint32_t* cur = reinterpret_cast<uint32_t*>(dl);  // [D] per sorted key
  uint32_t carry = 0;
  for (uint32_t j0 = 0; j0 < D; j0 += kBkThr) {
    const uint32_t j = j0 + t;
    const uint64_t v = j < D ? hs[j] : 0ull;
    const uint32_t cnt = (uint32_t)(v >> 16) & 0xffffu;
    uint32_t tot;
    const uint32_t ex = tp_block_scan<kBkThr>(cnt, lds, &tot) + carry;
    if (j < D) {
      const int64_t u = (int64_t)ubase + j;
      if (in_range(u, u_cap)) {
        uniq[u] = key0 | (uint32_t)(v >> 32);
        seg_start[u] = (int32_t)(ebase + ex);
        if (zero_a) zero_a[u] = 0.f;
        if (zero_b) zero_b[u] = 0ull;
      }
      cur[j] = ex;
    }
    carry += tot;
  }
  __syncthreads();
  for (uint32_t g = t; g < E; g += kBkThr) {
    const int32_t id = locate(g);
    const uint32_t key = tkeys[id] | (hb << shift);
    uint32_t lo = 0, up = D - 1;  // the sorted key's index
    while (lo < up) {
      const uint32_t mid = (lo + up) >> 1;
      if ((uint32_t)(hs[mid] >> 32) < key) lo = mid + 1; else up = mid;
    }
    if (D == 0 || (uint32_t)(hs[lo] >> 32) != key) continue;  // (only after an overflow)
    const uint32_t pos = atomicAdd(&cur[lo], 1u);
    const uint32_t u = ubase + lo;
    const int64_t e = (int64_t)ebase + pos;
    if (in_range(e, e_cap)) {
      pos_s[e] = id;
      segid[e] = (int32_t)(u + 1);
    }
    if (in_range((int64_t)id, e_cap)) ent_uid[id] = (int32_t)u;
  }
  __syncthreads();
}

// One workgroup per pair of fine buckets (pair = false: per fine bucket). The status
// words are per FINE bucket: a pair publishes its counts at 2b and an empty aggregate at
// 2b+1, so the look-back sums the same either way. A pair that overflows the LDS
// capacity or its hash (nearly distinct keys) processes its two fine buckets one after
// the other instead (tp_bk_fine_light), each with its own publish and look-back; the
// fine geometry keeps that exact even when every key is distinct. (Tried and dropped:
// redoing the whole launch in a gated fine-bucket kernel, +4.8 us per step for the
// empty launch; the fallback as a second copy of the register-staged path, 95 VGPRs.)
// (8 waves per SIMD = 4 workgroups per CU: <= 64 VGPRs)
__global__ void __launch_bounds__(tp::kBkThr, 8)
tp_bucket_kernel(const uint32_t* __restrict__ tkeys, const uint16_t* __restrict__ toff, int nbf,
                 int pair, int T, int shift, uint64_t* __restrict__ status,
                 uint32_t* __restrict__ epoch, int32_t* __restrict__ pos_s,
                 int32_t* __restrict__ segid, uint64_t* __restrict__ uniq,
                 int32_t* __restrict__ seg_start, int32_t* __restrict__ ent_uid,
                 int32_t* __restrict__ n_uniq, int32_t* __restrict__ n_ent,
                 float* __restrict__ zero_a, unsigned long long* __restrict__ zero_b,
                 int64_t u_cap, int64_t e_cap, int32_t* __restrict__ err,
                 uint64_t* __restrict__ prof) {
  using namespace tp;
  // 40,960 B of LDS (<= 40 KB: 4 workgroups of 512 threads per CU)
  __shared__ uint16_t eh[kECapL];   // hash slot of every gathered entry
  __shared__ uint64_t hs[kDH];      // hash (key u32 | count u32), then the sorted list
  __shared__ uint64_t dl[kDH];      // per-tile runs (until the inserts), then compacted
                                    // (key | count << 16 | slot), then cur/jj
  __shared__ uint32_t lds[kBkThr / 64 + 1];
  __shared__ uint32_t sb[4];        // epoch, unique base, entry base, build flag
  static_assert((kMaxT + 1) * 4 + kMaxT * 4 <= kDH * 8, "tile runs must fit in dl");
  uint32_t* hkey = reinterpret_cast<uint32_t*>(hs);
  uint32_t* hcnt = hkey + kDH;
  const int t = threadIdx.x, b = blockIdx.x;
  if (prof && t == 0) {
    prof[(int64_t)b * 12 + 0] = clock64();
    prof[(int64_t)b * 12 + 8] = __builtin_amdgcn_s_memrealtime();
  }
  if (t == 0) {
    uint32_t ep = (__hip_atomic_load(epoch, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) + 1u) & 0xffu;
    sb[0] = ep ? ep : 1u;
  }
  const int f0 = pair ? 2 * b : b, twin = pair ? f0 + 1 : f0;
  const uint64_t key0 = (uint64_t)f0 << shift;
  int32_t idx[kG];
  uint32_t E, D;
  const bool good = tp_bk_build(tkeys, toff, nbf, T, shift, f0, pair ? 2 : 1, 0u, hkey, hcnt, dl,
                                eh, lds, &sb[3], idx, &E, &D, prof);
  const uint32_t ep = sb[0];
  if (!good && pair) {
#pragma unroll 1
    for (int s = 0; s < 2; ++s)
      tp_bk_fine_light(tkeys, toff, nbf, T, shift, f0 + s, (uint32_t)s, key0, hkey, hcnt, hs, dl,
                       eh, lds, sb, status, ep, epoch, pos_s, segid, uniq, seg_start, ent_uid,
                       n_uniq, n_ent, zero_a, zero_b, u_cap, e_cap, err);
    return;
  }
  if (!good && t == 0) atomicOr(err, 1);
  if (t == 0) {  // publish (fine bucket 0: its inclusive prefix); a pair's twin is empty
    if (twin != f0)
      __hip_atomic_store(&status[twin], tp_status(ep, kStA, 0, 0), __ATOMIC_RELAXED,
                         __HIP_MEMORY_SCOPE_AGENT);
    __hip_atomic_store(&status[f0], tp_status(ep, f0 == 0 ? kStP : kStA, D, E), __ATOMIC_RELAXED,
                       __HIP_MEMORY_SCOPE_AGENT);
  }
  if (prof && t == 0) prof[(int64_t)b * 12 + 3] = clock64();
  tp_bk_ranksort(dl, hs, D);
  if (prof && t == 0) prof[(int64_t)b * 12 + 4] = clock64();
  tp_bk_lookback(status, f0, twin, nbf, ep, D, E, sb, epoch, n_uniq, n_ent, seg_start, u_cap, err);
  __syncthreads();
  if (prof && t == 0) prof[(int64_t)b * 12 + 5] = clock64();
  tp_bk_emit(hs, dl, eh, idx, D, sb[1], sb[2], key0, lds, pos_s, segid, uniq, seg_start, ent_uid,
             zero_a, zero_b, u_cap, e_cap, prof);
  if (prof && t == 0) {
    prof[(int64_t)b * 12 + 7] = clock64();
    prof[(int64_t)b * 12 + 9] = __builtin_amdgcn_s_memrealtime();
  }
}

// ------------------------------------------------------------- flat ("tpf") bucket
// (the layout these write -- fixed per-workgroup regions -- is described in tploc.cuh)
// Overflow unit (an overflowing pair's fine bucket f, or a lone bucket whose entries
// exceed the LDS capacity): register-light like tp_bk_fine_light; entries are located
// again from the per-tile runs for every pass, their key index found by probing the hash.
// Writes D / E into co[0..1] and returns E (block-uniform, via lds).
__device__ __forceinline__ uint32_t tpf_unit_light(
    const uint32_t* __restrict__ tkeys, const uint16_t* __restrict__ toff, int nbf, int T,
    int shift, int f, uint32_t hb, uint64_t key0, uint32_t* hkey, uint32_t* hmap,
    uint16_t* ehraw, uint32_t* lds, uint64_t* __restrict__ uo, int32_t* __restrict__ po,
    uint16_t* __restrict__ jo, uint32_t eoff, int32_t* __restrict__ co,
    int32_t* __restrict__ err, bool sorted) {
  using namespace tp;
  const int t = threadIdx.x;
  uint32_t* tpre = reinterpret_cast<uint32_t*>(ehraw);             // [kMaxT + 1]
  uint16_t* tlo = reinterpret_cast<uint16_t*>(tpre + kMaxT + 1);  // [kMaxT]
  for (int s = t; s < kDH; s += kBkThr) hkey[s] = kEmpty;
  const int per = (T + kBkThr - 1) / kBkThr;
  const int q0 = t * per, q1 = q0 + per < T ? q0 + per : T;
  uint32_t c = 0;
  for (int q = q0; q < q1; ++q) {
    const uint16_t* to = toff + (int64_t)q * (nbf + 1);
    const uint32_t lo = to[f], hi = to[f + 1];
    tlo[q] = (uint16_t)lo;
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
  auto locate = [&](uint32_t g) -> int32_t {
    int lo = 0, up = T - 1;  // last tile with tpre[q] <= g
    while (lo < up) {
      const int mid = (lo + up + 1) >> 1;
      if (tpre[mid] <= g) lo = mid; else up = mid - 1;
    }
    return lo * kTile + tlo[lo] + (int32_t)(g - tpre[lo]);
  };
  // probe (insert = true: claim an empty slot); returns the slot or -1
  auto probe = [&](uint32_t key, bool insert) -> int {
    uint32_t h = tp_hash(key) & (kDH - 1);
    for (int p = 0; p < kDH; ++p) {
      const uint32_t cu = hkey[h];
      if (cu == key) return (int)h;
      if (cu == kEmpty) {
        if (!insert) return -1;
        const uint32_t prev = atomicCAS(&hkey[h], kEmpty, key);
        if (prev == kEmpty || prev == key) return (int)h;
      }
      h = (h + 1) & (kDH - 1);
    }
    return -1;
  };
  bool bad = false;
  // 4 entries per thread per round: every locate, then every key load in flight, then the
  // probes (one memory round trip per round instead of one per entry)
  constexpr int kLB = 4;
  for (uint32_t c0 = 0; c0 < E; c0 += kBkThr * kLB) {
    int32_t id[kLB];
    uint32_t kk[kLB];
#pragma unroll
    for (int q = 0; q < kLB; ++q) {
      const uint32_t g = c0 + q * kBkThr + t;
      id[q] = locate(g < E ? g : E - 1);
    }
#pragma unroll
    for (int q = 0; q < kLB; ++q) kk[q] = tkeys[id[q]];
#pragma unroll
    for (int q = 0; q < kLB; ++q)
      if (c0 + q * kBkThr + t < E) bad |= probe(kk[q] | (hb << shift), true) < 0;
  }
  __syncthreads();
  // key index j of every occupied slot (strided: conflict-free LDS reads): compaction
  // order, or (sorted) the key's rank = # smaller keys of the unit (the keys are
  // distinct and below kEmpty)
  constexpr int kPer = kDH / kBkThr;
  uint32_t cc = 0;
#pragma unroll
  for (int q = 0; q < kPer; ++q) cc += hkey[q * kBkThr + t] != kEmpty;
  uint32_t D;
  uint32_t wd = tp_block_scan<kBkThr>(cc, lds, &D);
#pragma unroll
  for (int q = 0; q < kPer; ++q) {
    const int s = q * kBkThr + t;
    const uint32_t k = hkey[s];
    if (k != kEmpty) {
      uint32_t j = wd++;
      if (sorted) {
        j = 0;
        for (int r = 0; r < kDH; ++r) j += hkey[r] < k;  // (kEmpty is never < k)
      }
      hmap[s] = j;
      uo[j] = key0 | k;
    }
  }
  __syncthreads();
  const uint32_t room = eoff < (uint32_t)tpf::kEC ? tpf::kEC - eoff : 0u;
  bad |= E > room;
  const uint32_t Er = E < room ? E : room;
  for (uint32_t c0 = 0; c0 < Er; c0 += kBkThr * kLB) {
    int32_t id[kLB];
    uint32_t kk[kLB];
#pragma unroll
    for (int q = 0; q < kLB; ++q) {
      const uint32_t g = c0 + q * kBkThr + t;
      id[q] = locate(g < Er ? g : Er - 1);
    }
#pragma unroll
    for (int q = 0; q < kLB; ++q) kk[q] = tkeys[id[q]];
#pragma unroll
    for (int q = 0; q < kLB; ++q) {
      const uint32_t g = c0 + q * kBkThr + t;
      if (g >= Er) continue;
      const int h = probe(kk[q] | (hb << shift), false);
      po[eoff + g] = id[q];
      jo[eoff + g] = h >= 0 ? (uint16_t)hmap[h] : (uint16_t)0;
    }
  }
  if (bad) atomicOr(err, 1);
  if (t == 0) {
    co[0] = (int32_t)D;
    co[1] = (int32_t)(E < room ? E : room);
  }
  __syncthreads();
  return E < room ? E : room;
}

// Rank order of a unit's distinct keys by counting them into 256 bins of their top bits
// (the mixed keys are uniform over the unit's range [0, 2^kbits)) and comparing each key
// with the few others of its bin: O(D) work and 5 barriers instead of tp_bk_ranksort's
// O(D^2) scan. In: dl[0..D) (key u32 << 32 | count | slot). Out: dl[0..D) in key order.
// Scratch: sc = the dead hash region (>= kDH + 514 words: bin keys, counts, starts).
__device__ __forceinline__ void tpf_rank_binned(uint64_t* dl, uint32_t* sc, uint32_t D, int kbits,
                                                uint32_t* lds) {
  using namespace tp;
  constexpr int kPerT = kDH / kBkThr;  // <= 4 keys per thread
  const int t = threadIdx.x;
  const int bsh = kbits > 8 ? kbits - 8 : 0;
  uint32_t* bkey = sc;              // [kDH] keys grouped by bin
  uint32_t* bcnt = sc + kDH;        // [256]
  uint32_t* bst = bcnt + 256;       // [256] bin starts
  if (t < 256) bcnt[t] = 0u;
  __syncthreads();
  uint64_t e[kPerT];
  uint32_t bs[kPerT];  // bin << 16 | slot in bin
#pragma unroll
  for (int q = 0; q < kPerT; ++q) {
    const uint32_t i = q * kBkThr + t;
    e[q] = i < D ? dl[i] : 0ull;
    if (i < D) {
      const uint32_t bin = ((uint32_t)(e[q] >> 32) >> bsh) & 255u;
      bs[q] = bin << 16 | atomicAdd(&bcnt[bin], 1u);
    }
  }
  __syncthreads();
  uint32_t tot;
  const uint32_t st = tp_block_scan<kBkThr>(t < 256 ? bcnt[t] : 0u, lds, &tot);
  if (t < 256) bst[t] = st;
  __syncthreads();
#pragma unroll
  for (int q = 0; q < kPerT; ++q)
    if (q * kBkThr + t < D) bkey[bst[bs[q] >> 16] + (bs[q] & 0xffffu)] = (uint32_t)(e[q] >> 32);
  __syncthreads();
  uint32_t rk[kPerT];
#pragma unroll
  for (int q = 0; q < kPerT; ++q) {
    if (q * kBkThr + t >= D) continue;
    const uint32_t bin = bs[q] >> 16, a = bst[bin], n = bcnt[bin];
    const uint32_t k = (uint32_t)(e[q] >> 32);
    uint32_t r = a;
    for (uint32_t m = 0; m < n; ++m) r += bkey[a + m] < k;  // distinct keys
    rk[q] = r;
  }
  __syncthreads();  // (every dl entry is in registers: dl takes the ordered list)
#pragma unroll
  for (int q = 0; q < kPerT; ++q)
    if (q * kBkThr + t < D) dl[rk[q]] = e[q];
  __syncthreads();
}

// One workgroup per pair of fine buckets (pair = 0: per fine bucket), the tp_bucket
// geometry and build; the occupied hash slots in compaction order are the keys' indices.
// kFilt (tail filter, count mode): the LDS build sums the tile kernel's per-entry
// occurrence counts, and each key of a built unit carries its count (a byte) in the top
// byte of uniqf for tpf_filter_kernel, which runs as its own launch so that only IT has to
// run in minibatch order.
template <bool kFilt>
__global__ void __launch_bounds__(tp::kBkThr, 8)
tpf_bucket_kernel(const uint32_t* __restrict__ tkeys, const uint16_t* __restrict__ toff, int nbf,
                  int pair, int T, int shift, uint64_t* __restrict__ uniqf,
                  int32_t* __restrict__ ent_pos, uint16_t* __restrict__ ent_j,
                  int32_t* __restrict__ cnt, int32_t* __restrict__ err, int sorted,
                  const uint8_t* __restrict__ ecnt) {
  using namespace tp;
  __shared__ alignas(16) uint16_t eh[kECapL];  // hash slot of every gathered entry
  __shared__ uint64_t hs[kDH];     // hash (key u32 | count u32 -> key index)
  __shared__ uint64_t dl[kDH];     // per-tile runs, then the compacted occupied slots
  __shared__ uint32_t lds[kBkThr / 64 + 1];
  __shared__ uint32_t flag;
  uint32_t* hkey = reinterpret_cast<uint32_t*>(hs);
  uint32_t* hcnt = hkey + kDH;
  const int t = threadIdx.x, b = blockIdx.x;  // (tpf_xcd_group_of: measured and not kept)
  const int f0 = pair ? 2 * b : b;
  const uint64_t key0 = (uint64_t)f0 << shift;
  uint64_t* uo = uniqf + (int64_t)b * tpf::kUC;
  int32_t* po = ent_pos + (int64_t)b * tpf::kEC;
  uint16_t* jo = ent_j + (int64_t)b * tpf::kEC;
  int32_t* co = cnt + (int64_t)b * 4;
  int32_t idx[kG];
  uint32_t E, D;
  const bool good = tp_bk_build<kFilt>(tkeys, toff, nbf, T, shift, f0, pair ? 2 : 1, 0u, hkey,
                                       hcnt, dl, eh, lds, &flag, idx, &E, &D, nullptr, ecnt);
  if (good) {
    // key index j: compaction order, or (sorted: the multi-GPU exchange rows must be
    // key-ordered) the rank order of tp_bk_ranksort; slot -> j in LDS (the dead hash
    // counts, or the dead compaction list once it is sorted into hs)
    uint32_t* jmap = hcnt;
    const uint64_t* lst = dl;
    if (sorted && D > 64) {  // binned rank order into dl; the dead hash takes slot -> j
      tpf_rank_binned(dl, hkey, D, pair ? shift + 1 : shift, lds);
      jmap = hkey;
    } else if (sorted) {
      tp_bk_ranksort(dl, hs, D);
      __syncthreads();
      jmap = reinterpret_cast<uint32_t*>(dl);
      lst = hs;
    }
    for (uint32_t j = t; j < D; j += kBkThr) {
      const uint64_t v = lst[j];
      // (tail filter: the key's occurrences, saturated to a byte, ride in the top byte
      // until the filter rewrites the unit's keys)
      uo[j] = key0 | (uint32_t)(v >> 32) |
              (kFilt ? (uint64_t)min((uint32_t)(v >> 16) & 0xffffu, 255u) << 56 : 0ull);
      jmap[(uint32_t)v & 0xffffu] = j;
    }
    __syncthreads();
#pragma unroll
    for (int q = 0; q < kG; ++q) {
      if (idx[q] < 0) continue;
      const uint32_t g = q * kBkThr + t;
      po[g] = idx[q];
      jo[g] = (uint16_t)jmap[eh[g]];
    }
    if (t == 0) {
      co[0] = (int32_t)D;
      co[1] = (int32_t)E;
      co[2] = 0;
      co[3] = 0;
    }
  } else {
    // the pair's entries overflow the LDS capacity or its hash (near-distinct keys; the
    // hash build gives up after kBkProbe probes): its fine buckets one after the other,
    // each a unit with its own key index space. (Measured and not kept: the LDS build per
    // fine bucket here -- as a second inlined build it spilled the main path, as a
    // non-inlined call (308 B of scratch) it slowed the headline step 0.082 -> 0.105 ms,
    // profiles/r6_skew_layout.log.)
    {
      const uint32_t e0 = tpf_unit_light(tkeys, toff, nbf, T, shift, f0, 0u, key0, hkey, hcnt, eh,
                                         lds, uo, po, jo, 0u, co, err, sorted != 0);
      if (pair)
        tpf_unit_light(tkeys, toff, nbf, T, shift, f0 + 1, 1u, key0, hkey, hcnt, eh, lds,
                       uo + tpf::kUnitK, po, jo, e0, co + 2, err, sorted != 0);
      else if (t == 0) {
        co[2] = 0;
        co[3] = 0;
      }
    }
  }
}

// ------------------------------------------------------------------- host side
// temp's first (nbk * 8 + 16) bytes (status words + epoch) must be zero before the
// first launch (the Python side allocates it zeroed); they need no reset afterwards
void localize_tp(const uint64_t* raw, int64_t n, KeyMix m, void* temp, size_t temp_bytes,
                 int32_t* dcnt, uint16_t* rep, int32_t* pos_s, int32_t* segid, uint64_t* uniq,
                 int32_t* seg_start, int32_t* ent_uid, int32_t* local_col, int32_t* n_uniq,
                 int32_t* n_ent, float* grad, unsigned long long* pieces, int32_t* err,
                 int64_t u_cap, uint64_t* prof, hipStream_t st) {
  if (n <= 0) return;
  if (!tploc_supported(n, m.bits)) throw std::runtime_error("localize_tp: unsupported size");
  if (temp_bytes < tploc_temp_bytes(n, m.bits)) throw std::runtime_error("localize_tp: temp");
  const TpGeom g = tp_geom(n, m.bits);
  char* p = (char*)temp;
  auto take = [&](size_t bytes) { char* r = p; p += al16(bytes); return r; };
  uint64_t* status = (uint64_t*)take((size_t)g.nbk * 8 + 16);
  uint32_t* epoch = (uint32_t*)(status + g.nbk);
  uint32_t* tkeys = (uint32_t*)take((size_t)g.N * 4);
  uint16_t* toff = (uint16_t*)take((size_t)g.T * (g.nbk + 1) * 2);
  tp_launch_tile(raw, n, m, g, tkeys, toff, dcnt, rep, err, nullptr, st);
  // buckets in pairs of fine buckets: one round of workgroups (the pair's key bit above
  // a <= 30-bit suffix keeps the LDS hash's empty word unreachable)
  const bool pair = g.nbk >= 2 && g.shift <= 30;
  tp_bucket_kernel<<<(unsigned)(pair ? g.nbk / 2 : g.nbk), tp::kBkThr, 0, st>>>(
      tkeys, toff, g.nbk, pair ? 1 : 0, (int)g.T, g.shift, status, epoch, pos_s, segid, uniq,
      seg_start, ent_uid, n_uniq, n_ent, grad, pieces, u_cap, g.N, err, prof);
  PSAMD_HIP_CHECK(hipGetLastError());
  // (skipped when the fused forward reads the entry map directly)
  if (local_col) tp_gather(rep, ent_uid, n, local_col, st);
}

void tpf_launch_bucket(const TpGeom& g, const uint32_t* tkeys, const uint16_t* toff,
                       uint64_t* uniqf, int32_t* ent_pos, uint16_t* ent_j, int32_t* cnt,
                       int32_t* err, bool sorted, const uint8_t* ecnt, hipStream_t st) {
  const int pair = tpf_pair(g) ? 1 : 0;
  if (ecnt)
    tpf_bucket_kernel<true><<<(unsigned)tpf_groups_of(g), tp::kBkThr, 0, st>>>(
        tkeys, toff, g.nbk, pair, (int)g.T, g.shift, uniqf, ent_pos, ent_j, cnt, err,
        sorted ? 1 : 0, ecnt);
  else
    tpf_bucket_kernel<false><<<(unsigned)tpf_groups_of(g), tp::kBkThr, 0, st>>>(
        tkeys, toff, g.nbk, pair, (int)g.T, g.shift, uniqf, ent_pos, ent_j, cnt, err,
        sorted ? 1 : 0, nullptr);
  PSAMD_HIP_CHECK(hipGetLastError());
}

}  // namespace psamd
