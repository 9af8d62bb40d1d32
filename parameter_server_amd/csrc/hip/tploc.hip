// Localisation by tile dedup + bucket partition ("tp", mixed key spaces <= 34 bits,
// <= 5.2 M keys per minibatch: tploc_supported; the Localizer sorts anything larger).
//
// Reference: Localizer::countUniqIndex / remapIndex (src/util/localizer.h:69-191) sort
// every (key, position) pair of a minibatch and rebuild a CSR with local ids.
//
// Measured on MI355X for a 65,536 x 39 Criteo-shaped minibatch (2.56 M keys, 234 K
// distinct): 1 944 hot keys hold 77 % of the occurrences, and a full LSD radix sort
// (sort32.hip) is 16 small launches, ~200 us. Device-scope atomics run at ~20 per
// ns (benchmarks/probe_atomics.py), so a global hash with per-key atomics cannot beat
// it either. This path touches each occurrence once, in LDS, and works on the
// tile-distinct "entries" (~1 M) afterwards, with no global atomics at all:
//
//   tile     one 1024-thread workgroup per tile of 8192 occurrences: mix, LDS hash
//            dedup, counting sort of the tile's distinct keys by bucket (top BB key
//            bits) -> tkeys[tile][pos], per-tile bucket offsets toff[tile][b],
//            rep[i] = tile entry of occurrence i (u16)
//   bucket   (tploc_bucket.hip) one workgroup per bucket: the bucket's entries from
//            every tile -> distinct keys, and either the compact sorted layout ("tp")
//            or fixed per-workgroup regions (the flat 1-GPU layout, "tpf")
//   gather   local_col[i] = ent_uid[tile * 8192 + rep[i]]
//
// Buckets are ranges of the mixed key space, so the unique keys come out sorted
// (the multi-GPU owner split and the ordered home slots of the KV table rely on it).
//
// This unit: the tile kernel (both layouts launch it through tp_launch_tile), the gather
// kernel and the host geometry of the family. The other units: tploc_bucket.hip (bucket
// kernels of both layouts), tploc_flat.hip (the flat layout's tail filter, localize_tpf),
// tploc_fused.hip (forward / backward on either layout), tploc_step.hip (the flat step
// boundary and exchange); tploc.cuh holds the device helpers they share, tploc_geom.h the
// host ones.
#include "tploc.cuh"
#include "tploc_geom.h"

#include <algorithm>
#include <cstdlib>

namespace psamd {

// ------------------------------------------------------------------------ tile
// Phase marks of the tile kernel (a tuning aid, benchmarks/prof_tile_phases.py): null
// unless tp_tile_set_prof() installed a buffer of 16 u64 per workgroup.
__device__ uint64_t* g_tile_prof = nullptr;
#define TILE_MARK(k)                                                            \
  if (tpp && threadIdx.x == 0) tpp[(int64_t)blockIdx.x * 16 + (k)] = clock64()

// kQuot = false (<= 31-bit keys): the slot keeps the key itself, home = low kHB key bits;
// kQuot = true (32..34 bits): quotient encoding, home = low kHB key bits.
// kCnt (the tail filter's counts): ecnt[tile * kTile + e] = occurrences of entry e in the
// tile, saturated to a byte (LDS u16 pairs in the dead hash, one integer LDS add per
// occurrence).
// (8 waves per SIMD = 2 workgroups per CU: <= 64 VGPRs. The quotient variant compiled to
// 66 without the bound, i.e. 1 workgroup per CU: localise 90 vs 80 us.)
template <bool kQuot, bool kCnt = false>
__global__ void __launch_bounds__(tp::kThr, 8)
tp_tile_kernel(const uint64_t* __restrict__ raw, int64_t n, KeyMix m, int shift, int nbk,
               uint32_t* __restrict__ tkeys, uint16_t* __restrict__ toff,
               int32_t* __restrict__ dcnt, uint16_t* __restrict__ rep,
               int32_t* __restrict__ err, int lts, uint8_t* __restrict__ ecnt = nullptr) {
  using namespace tp;
  __shared__ uint32_t hk[kHash];    // quotient-encoded keys; after the bucket sort: entry position
  __shared__ uint32_t cnt[kMaxBk];  // per-bucket counts, then offsets
  __shared__ uint32_t lds[kThr / 64 + 1];
  const int t = threadIdx.x;
  uint64_t* const tpp = g_tile_prof;
  if (tpp && t == 0) tpp[(int64_t)blockIdx.x * 16 + 8] = __builtin_amdgcn_s_memrealtime();
  TILE_MARK(0);
  for (int i = t; i < kHash; i += kThr) hk[i] = kEmpty;
  for (int d = t; d < nbk; d += kThr) cnt[d] = 0;
  __syncthreads();
  TILE_MARK(1);
  // occurrences [base, base + lim) (2^lts per tile, tp_geom); entry ids keep the
  // kTile stride (tkeys, dcnt, the consumers' tile * kTile + entry)
  const int64_t base = (int64_t)blockIdx.x << lts;
  const int lim = (int)(n - base < (1 << lts) ? n - base : (1 << lts));
  uint64_t kr[kIt];  // raw keys, then the mixed keys
  uint16_t sl[kIt];  // hash slot of every key
  uint32_t rr[kIt];  // a key this lane inserted (one lane per distinct key): rank in its
                     // bucket, then its entry position; kEmpty otherwise
  uint32_t won = 0;  // bit j: this lane inserted key j
  bool bad = false;
#pragma unroll
  for (int j = 0; j < kIt; ++j) {  // all loads in flight before the LDS insert chain
    const int o = j * kThr + t;
    kr[j] = o < lim ? raw[base + o] : 0ull;
  }
  if (tpp) {  // (profiling only: every load landed, workgroup-wide)
    __builtin_amdgcn_s_waitcnt(0);
    __syncthreads();
    TILE_MARK(2);
  }
  // (<= 31 bits: the mix in 32-bit arithmetic -- the low bits of a product depend only
  // on the low bits of its factors, so it equals mix_key -- and the mixed key's own low
  // bits as the home slot: ~12 fewer VALU per key than the 64-bit mix + tp_hash. Measured
  // and not kept: two keys per probe loop, both probes' LDS reads and CAS in flight
  // together: insert phase 19.1 -> 22.2 k cycles per workgroup, benchmarks/prof_tile_phases.py)
#pragma unroll
  for (int j = 0; j < kIt; ++j) {
    sl[j] = 0;
    if (j * kThr + t < lim) {
      const uint64_t k = kQuot ? mix_key(kr[j], m) : (uint64_t)mix_key32(kr[j], m);
      kr[j] = k;
      const uint32_t q = kQuot ? (uint32_t)(k >> kHB) << kDispB : (uint32_t)k;
      uint32_t h = (uint32_t)k & (kHash - 1);
      uint32_t d = 0;
      for (; d < kMaxDisp; ++d) {  // slot h holds key k iff it holds q | d (q: kQuot = false)
        const uint32_t want = kQuot ? q | d : q;
        const uint32_t cur = hk[h];
        if (cur == want) break;
        if (cur == kEmpty) {
          const uint32_t prev = atomicCAS(&hk[h], kEmpty, want);
          if (prev == kEmpty) {
            won |= 1u << j;
            break;
          }
          if (prev == want) break;
        }
        h = (h + 1) & (kHash - 1);
      }
      bad |= d == kMaxDisp;
      sl[j] = (uint16_t)h;
    }
  }
  // counting sort of the distinct keys by bucket (top key bits), by the lanes that
  // inserted them: their keys are in registers, so no pass over the (mostly empty) hash
  // (the earlier form scanned all 16 K slots twice: ~3 K of them hold a key). The tile
  // keys leave as their low `shift` bits (the bucket holds the rest).
#pragma unroll
  for (int j = 0; j < kIt; ++j)
    rr[j] = (won >> j) & 1u ? atomicAdd(&cnt[kr[j] >> shift], 1u) : kEmpty;
  if (bad && err) atomicOr(err, 2);
  __syncthreads();
  TILE_MARK(3);
  // exclusive scan of the bucket counts (nbk <= kMaxBk: 2 per thread)
  constexpr int kDP = kMaxBk / kThr;
  uint32_t c[kDP], s = 0;
#pragma unroll
  for (int e = 0; e < kDP; ++e) {
    const int d = t * kDP + e;
    c[e] = d < nbk ? cnt[d] : 0u;
    s += c[e];
  }
  uint32_t D;
  uint32_t run = tp_block_scan<kThr>(s, lds, &D);
  uint16_t* to = toff + (int64_t)blockIdx.x * (nbk + 1);
#pragma unroll
  for (int e = 0; e < kDP; ++e) {
    const int d = t * kDP + e;
    if (d < nbk) {
      cnt[d] = run;
      to[d] = (uint16_t)run;
    }
    run += c[e];
  }
  if (t == 0) {
    to[nbk] = (uint16_t)D;
    dcnt[blockIdx.x] = (int32_t)D;
  }
  __syncthreads();
  TILE_MARK(4);
  // each inserted key -> its entry position: tile key out, and its hash slot now holds
  // the position (no lane reads hk between the two barriers)
  uint32_t* tk = tkeys + (int64_t)blockIdx.x * kTile;
  const uint64_t smask = (1ull << shift) - 1;
#pragma unroll
  for (int j = 0; j < kIt; ++j) {
    if (rr[j] != kEmpty) {
      const uint32_t pos = cnt[kr[j] >> shift] + rr[j];
      tk[pos] = (uint32_t)(kr[j] & smask);
      hk[sl[j]] = pos;
    }
  }
  __syncthreads();
  TILE_MARK(5);
#pragma unroll
  for (int j = 0; j < kIt; ++j) {
    const int o = j * kThr + t;
    if (o < lim) {
      const uint16_t pos = (uint16_t)hk[sl[j]];
      rep[base + o] = pos;
      if (kCnt) sl[j] = pos;
    }
  }
  if (kCnt) {  // occurrences per entry: u16 pairs in the dead hash
    __syncthreads();
    for (uint32_t i = t; i < (D + 1) / 2; i += kThr) hk[i] = 0u;
    __syncthreads();
#pragma unroll
    for (int j = 0; j < kIt; ++j)
      if (j * kThr + t < lim) atomicAdd(&hk[sl[j] >> 1], 1u << ((sl[j] & 1) * 16));
    __syncthreads();
    uint8_t* ec = ecnt + (int64_t)blockIdx.x * kTile;
    for (uint32_t i = t; i < D; i += kThr) {
      const uint32_t c = (hk[i >> 1] >> ((i & 1) * 16)) & 0xffffu;
      ec[i] = (uint8_t)(c > 255u ? 255u : c);
    }
  }
  if (tpp && t == 0) {
    TILE_MARK(6);
    tpp[(int64_t)blockIdx.x * 16 + 9] = __builtin_amdgcn_s_memrealtime();
    tpp[(int64_t)blockIdx.x * 16 + 10] = __smid();
  }
}
#undef TILE_MARK

void tp_tile_set_prof(uint64_t* p) {
  PSAMD_HIP_CHECK(hipMemcpyToSymbol(HIP_SYMBOL(g_tile_prof), &p, sizeof(p)));
}

// ---------------------------------------------------------------------- gather
__global__ void tp_gather_kernel(const uint16_t* __restrict__ rep,
                                 const int32_t* __restrict__ ent_uid, int64_t n,
                                 int32_t* __restrict__ local_col) {
  constexpr int kPer = 4;
  const int64_t i0 = (blockIdx.x * (int64_t)blockDim.x) * kPer + threadIdx.x;
  int64_t e[kPer];
#pragma unroll
  for (int q = 0; q < kPer; ++q) {
    const int64_t i = i0 + q * blockDim.x;
    e[q] = i < n ? (i / tp::kTile) * tp::kTile + rep[i] : -1;
  }
#pragma unroll
  for (int q = 0; q < kPer; ++q) {
    const int64_t i = i0 + q * blockDim.x;
    if (e[q] >= 0) local_col[i] = ent_uid[e[q]];
  }
}

// ------------------------------------------------------------------- host side
// Occurrences per tile of the FLAT layout, 2^lts in [1024, 8192]: the largest that still
// gives >= 128 tiles, so a small minibatch (B = 10,000 x 39: 48 tiles of 8192, i.e. 48
// busy CUs, each tile's LDS insert chain ~15 us) spreads over the chip; large ones keep
// 8192 (fewer tiles = fewer tile entries of the hot keys). Measured at B = 10,000
// (profiles/r5_adaptive_tiles.log): 8192 -> 260.6 M ex/s, 4096 -> 304.3, 2048 -> 309.3,
// 1024 -> 196.8 (the hot keys' extra entries). Entry ids keep the kTile stride whatever
// the tile holds. The compact "tp" layout always uses 8192.
// PSAMD_TILE_LTS=10..13 pins it (A/B), PSAMD_TILE_MIN the tile target.
int tp_flat_lts(int64_t n) {
  // (read per call: host-side geometry only, a few calls per launch list build)
  const char* pe = getenv("PSAMD_TILE_LTS");
  const int pin = pe ? atoi(pe) : 0;
  const char* te = getenv("PSAMD_TILE_MIN");
  int tmin = te ? atoi(te) : 128;
  tmin = tmin < 1 ? 1 : tmin > tp::kMaxT / 2 ? tp::kMaxT / 2 : tmin;
  int lts = 13;
  if (pin >= 10 && pin <= 13) {
    lts = pin;
  } else {
    while (lts > 10 && ((n + (1ll << lts) - 1) >> lts) < tmin) --lts;
  }
  while (lts < 13 && ((n + (1ll << lts) - 1) >> lts) > tp::kMaxT) ++lts;  // (LDS tile runs)
  return lts;
}

TpGeom tp_geom(int64_t n, int bits, bool flat) {
  TpGeom g;
  g.lts = flat ? tp_flat_lts(n) : 13;
  static_assert(tp::kTile == 8192, "tile entry stride 2^13");
  g.T = (n + (1ll << g.lts) - 1) >> g.lts;
  g.N = g.T * tp::kTile;
  // <= 1024 occurrences per bucket on average: even if every key is distinct a PAIR of
  // buckets (the flat layout's unit) stays under the kDH-key hash (at 1280, nearly
  // distinct minibatches -- e.g. 1000 rcv1-width rows over 10^8 ids -- overflowed every
  // pair into the register-light fallback: ~20x slower bucket kernel). The 2048-bucket
  // cap leaves the Criteo-shaped 65,536 x 39 batch as before (measured there: <= 1615
  // entries and 157 distinct keys per bucket at 2048 buckets)
  int bb = 0;
  while (bb < 11 && (n >> bb) > 1024) ++bb;
  if (bb > bits) bb = bits;
  g.nbk = 1 << bb;
  g.shift = bits - bb;
  return g;
}

int64_t tploc_stride(int64_t n) { return tp_geom(n, 31).N; }
// flat layout: the entry stride of an n-key minibatch, and a bound over every minibatch of
// <= n keys (a workspace sized for n must take smaller minibatches, which may use more,
// smaller tiles): <= kMaxT tiles, and tiles of 1024 at the least
int64_t tpf_stride(int64_t n) { return tp_geom(n, 31, true).N; }
int64_t tpf_stride_max(int64_t n) {
  const int64_t t = std::min<int64_t>(tp::kMaxT, (n + 1023) / 1024);
  return std::max<int64_t>(t, (n + tp::kTile - 1) / tp::kTile) * tp::kTile;
}
int tpf_tile_log2(int64_t n) { return tp_geom(n, 31, true).lts; }
int tploc_buckets(int64_t n, int bits) { return tp_geom(n, bits).nbk; }
int tploc_tile() { return tp::kTile; }

bool tploc_supported(int64_t n, int bits) {
  // <= 34 bits: quotient-encoded tile hash; bucket suffixes (bits - log2 nbk) < 32 bits
  return bits >= 2 && bits <= 34 && n > 0 && (n >> 11) <= 1280 &&
         (n + tp::kTile - 1) / tp::kTile <= tp::kMaxT && tp_geom(n, bits).shift <= 31;
}

size_t tploc_temp_bytes(int64_t n, int bits) {
  const TpGeom g = tp_geom(n, bits);
  return al16((size_t)g.nbk * 8 + 16)                          // look-back status + epoch
         + al16((size_t)g.N * 4)                               // tkeys
         + al16((size_t)g.T * (g.nbk + 1) * 2);                // toff (u16)
}

void tp_launch_tile(const uint64_t* raw, int64_t n, KeyMix m, const TpGeom& g, uint32_t* tkeys,
                    uint16_t* toff, int32_t* dcnt, uint16_t* rep, int32_t* err, uint8_t* ecnt,
                    hipStream_t st) {
  auto launch = [&](auto kernel) {
    kernel<<<(unsigned)g.T, tp::kThr, 0, st>>>(raw, n, m, g.shift, g.nbk, tkeys, toff, dcnt, rep,
                                               err, g.lts, ecnt);
  };
  const bool quot = m.bits > 31;
  if (quot && ecnt) launch(tp_tile_kernel<true, true>);
  else if (ecnt) launch(tp_tile_kernel<false, true>);
  else if (quot) launch(tp_tile_kernel<true, false>);
  else launch(tp_tile_kernel<false, false>);
  PSAMD_HIP_CHECK(hipGetLastError());
}

// ---- flat (tpf) geometry
int tpf_groups(int64_t n, int bits) { return tpf_groups_of(tp_geom(n, bits)); }
int tpf_key_region() { return tpf::kUC; }
int tpf_entry_region() { return tpf::kEC; }
int tpf_xcd_group(int bid, int groups) { return tpf_xcd_group_of(bid, groups); }

size_t tpf_temp_bytes(int64_t n, int bits) {  // (any minibatch of <= n keys: tpf_stride_max)
  const int64_t N = tpf_stride_max(n);
  return al16((size_t)N * 4) + al16((size_t)(N / tp::kTile) * (tp::kMaxBk + 1) * 2);  // tkeys, toff
}

void tp_gather(const uint16_t* rep, const int32_t* ent_uid, int64_t n, int32_t* local_col,
               hipStream_t st) {
  if (n <= 0) return;
  tp_gather_kernel<<<(unsigned)((n + 1023) / 1024), 256, 0, st>>>(rep, ent_uid, n, local_col);
  PSAMD_HIP_CHECK(hipGetLastError());
}

}  // namespace psamd
