// Flat ("tpf") localisation for one GPU: localize_tpf runs the tile stage of "tp"
// (tploc.hip), the flat bucket kernel (tploc_bucket.hip), which writes FIXED
// per-workgroup regions (described in tploc.cuh at namespace tpf) with no look-back and
// no CSC, and, with a tail filter, the filter kernel of this unit: the CountMin insert +
// query of the minibatch's keys (tpf_filter_unit: the sketch traffic staged in LDS,
// cm_stage_*, or with global atomics, tpf_filter_global) and the compaction of the kept
// keys and entries. The filter is a launch of its own so that only the sketch traffic has
// to run in minibatch order. Same limits as "tp": <= 34 key bits, <= 5.2 M keys
// (tploc_supported). Consumers of the layout: tploc_fused.hip, tploc_step.hip.
#include "tploc.cuh"
#include "tploc_geom.h"

#include <stdexcept>

namespace psamd {

// a unit key's bits (the bucket build's units carry the key's occurrences in the top byte
// until the tail filter rewrites them)
constexpr uint64_t kUoKey = (1ull << 56) - 1;

// The unit's sketch traffic with global atomics (units of more than kFlD keys, or k != 2):
// insert and query with the keys strided over the threads (key j = q * kBkThr + t), two
// keys at a time (4 spill past 64 VGPRs); keep flags -> occ[].
__device__ __forceinline__ void tpf_filter_global(const uint64_t* __restrict__ uo, uint32_t D,
                                                  const CmArgs& cm, uint32_t* occ) {
  using namespace tp;
  constexpr int kKP = tpf::kUnitK / kBkThr;
  const int t = threadIdx.x;
  auto load2 = [&](int hq, uint64_t (&k2)[2], uint32_t (&c2)[2]) -> uint32_t {
    uint32_t v = 0;
#pragma unroll
    for (int i = 0; i < 2; ++i) {
      const uint32_t j = (hq + i) * kBkThr + t;
      k2[i] = j < D ? uo[j] & kUoKey : 0ull;
      c2[i] = j < D ? (occ[j] > 255u ? 255u : occ[j]) : 0u;
      v |= (j < D ? 1u : 0u) << i;
    }
    return v;
  };
#pragma unroll
  for (int hq = 0; hq < kKP; hq += 2) {
    uint64_t k2[2];
    uint32_t c2[2];
    const uint32_t v = load2(hq, k2, c2);
    if (!v) continue;
    if (cm.k == kCmBatchK && cm.ncells32) {
      cm_insert_batch<2>(cm, k2, c2, v);
    } else {
      for (int i = 0; i < 2; ++i)
        if ((v >> i) & 1u) cm_insert_key(cm, k2[i], c2[i]);
    }
  }
  __syncthreads();  // every insert of this minibatch that can reach these keys' cells is done
#pragma unroll
  for (int hq = 0; hq < kKP; hq += 2) {
    uint64_t k2[2];
    uint32_t c2[2], e2[2] = {0u, 0u};
    const uint32_t v = load2(hq, k2, c2);
    if (!v) continue;
    if (cm.k == kCmBatchK && cm.ncells32) {
      cm_query_batch<2>(cm, k2, v, e2);
    } else {
      for (int i = 0; i < 2; ++i) e2[i] = (v >> i) & 1u ? cm_query_key(cm, k2[i]) : 0u;
    }
    // (each thread reads back only its own occ words: no barrier between the two)
    for (int i = 0; i < 2; ++i)
      if ((v >> i) & 1u) occ[(hq + i) * kBkThr + t] = (int)e2[i] > cm.freq ? 1u : 0u;
  }
}

// The unit's sketch traffic staged in LDS (units of <= kFlD keys, k = 2): the distinct
// sketch words of the unit's cells go into an LDS table (word index -> value), each
// loaded ONCE from HBM by the thread that claimed its slot; the saturating adds are LDS
// CAS loops, the queries read the table, and the changed words are written back with
// plain stores. Valid because this workgroup owns every region its keys map to
// (countmin.cuh) and no other kernel touches the sketch meanwhile (the tail-filtered
// pipelines order their bucket kernels): one memory round trip per key instead of the
// global form's load -> CAS -> reload chain (a device-scope atomic drops the line from the
// XCD's L2, MI355X_MICROARCH.md: the reload crosses the fabric again).
constexpr int kFlD = 1024;    // keys of a staged unit (occ_small: the dead entry-hash LDS)
constexpr int kFlTab = 4096;  // word table slots (load <= 0.5)

__device__ __forceinline__ void lds_sat_add_byte(uint32_t* w, uint32_t sh, uint32_t cnt,
                                                 uint32_t vmax) {
  uint32_t old = __hip_atomic_load(w, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
  while (true) {
    const uint32_t b = (old >> sh) & 0xffu;
    const uint32_t nb = (cnt > vmax - b) ? vmax : b + cnt;
    if (nb == b) return;
    const uint32_t prev = atomicCAS(w, old, (old & ~(0xffu << sh)) | (nb << sh));
    if (prev == old) return;
    old = prev;
  }
}

// (the staged form in two halves: claim + gathers in flight, issued before the unit's
// occurrence counting so the two memory round trips overlap; then adds, query, write-back)
struct CmStage {
  static constexpr int kQ = kFlD / tp::kBkThr;  // keys per thread (strided)
  uint32_t cell[kQ][kCmBatchK], g[kQ][kCmBatchK];
  uint32_t sl[kQ];         // the two probes' table slots, 16 bits each
  uint32_t mine, valid;    // (packed: registers are live across the occurrence counting)
  __device__ __forceinline__ uint32_t slot(int q, int p) const {
    return (sl[q] >> (16 * p)) & 0xffffu;
  }
};

__device__ __forceinline__ void cm_stage_begin(const uint64_t* __restrict__ uo, uint32_t D,
                                               const CmArgs& cm, uint32_t* wkey, CmStage& st,
                                               uint32_t* occ_packed) {
  using namespace tp;
  constexpr int kQ = CmStage::kQ;
  const int t = threadIdx.x;
  uint64_t k[kQ];
  st.valid = 0;
  st.mine = 0;
#pragma unroll
  for (int q = 0; q < kQ; ++q) {
    const uint32_t j = q * kBkThr + t;
    const uint64_t raw = uo[j < D ? j : 0];  // (D >= 1 here; clamped, unconditional loads)
    k[q] = raw & kUoKey;
    // (packed unit: the key's occurrence count rides in the top byte -- no second pass)
    if (occ_packed && j < D) occ_packed[j] = (uint32_t)(raw >> 56);
    st.valid |= (j < D ? 1u : 0u) << q;
  }
  cm_cells_batch<kQ>(cm, k, st.cell);
#pragma unroll
  for (int q = 0; q < kQ; ++q)
#pragma unroll
    for (int p = 0; p < kCmBatchK; ++p) {
      if (p == 0) st.sl[q] = 0;
      if (!((st.valid >> q) & 1u)) continue;
      const uint32_t w1 = (st.cell[q][p] >> 2) + 1u;  // (< 2^30 words: ncells32)
      uint32_t h = (w1 * 0x9E3779B1u) >> (32 - 12);
      static_assert(kFlTab == 1 << 12, "table hash width");
      while (true) {
        const uint32_t prev = atomicCAS(&wkey[h], 0u, w1);
        if (prev == 0u) {
          st.mine |= 1u << (q * kCmBatchK + p);
          break;
        }
        if (prev == w1) break;
        h = (h + 1) & (kFlTab - 1);
      }
      st.sl[q] |= h << (16 * p);
    }
#pragma unroll
  for (int q = 0; q < kQ; ++q)
#pragma unroll
    for (int p = 0; p < kCmBatchK; ++p)  // (every claimed word's load in flight)
      st.g[q][p] = (st.mine >> (q * kCmBatchK + p)) & 1u
                       ? __hip_atomic_load(cm.cells + (st.cell[q][p] >> 2), __ATOMIC_RELAXED,
                                           __HIP_MEMORY_SCOPE_AGENT)
                       : 0u;
}

__device__ __forceinline__ void cm_stage_end(const CmArgs& cm, uint32_t* occ, uint32_t* wval,
                                             CmStage& st) {
  using namespace tp;
  constexpr int kQ = CmStage::kQ;
  const int t = threadIdx.x;
#pragma unroll
  for (int q = 0; q < kQ; ++q)
#pragma unroll
    for (int p = 0; p < kCmBatchK; ++p)
      if ((st.mine >> (q * kCmBatchK + p)) & 1u) wval[st.slot(q, p)] = st.g[q][p];
  __syncthreads();
#pragma unroll
  for (int q = 0; q < kQ; ++q) {
    if (!((st.valid >> q) & 1u)) continue;
    const uint32_t o = occ[q * kBkThr + t];
    const uint32_t c = o > 255u ? 255u : o;
#pragma unroll
    for (int p = 0; p < kCmBatchK; ++p)
      lds_sat_add_byte(&wval[st.slot(q, p)], (st.cell[q][p] & 3u) * 8u, c, cm.vmax);
  }
  __syncthreads();  // every insert of the unit is in the table
#pragma unroll
  for (int q = 0; q < kQ; ++q) {
    if (!((st.valid >> q) & 1u)) continue;
    uint32_t r = cm.vmax;
#pragma unroll
    for (int p = 0; p < kCmBatchK; ++p) {
      const uint32_t v = (wval[st.slot(q, p)] >> ((st.cell[q][p] & 3u) * 8u)) & 0xffu;
      r = v < r ? v : r;
    }
    occ[q * kBkThr + t] = (int)r > cm.freq ? 1u : 0u;  // (own occ words: read above)
  }
#pragma unroll
  for (int q = 0; q < kQ; ++q)
#pragma unroll
    for (int p = 0; p < kCmBatchK; ++p)
      if ((st.mine >> (q * kCmBatchK + p)) & 1u) {
        const uint32_t v = wval[st.slot(q, p)];
        if (v != st.g[q][p]) cm.cells[st.cell[q][p] >> 2] = v;
      }
}

// Fused tail-feature filter of one unit of the flat layout (reference
// MinibatchReader::read, src/learner/sgd.h:131-150: CountMin insertKeys of the minibatch's
// per-key counts, then queryKeys > tail_feature_freq, src/parameter/frequency_filter.h:
// 26-45). In: keys uo[0..D), entries po / jo[ein .. ein + E) (jo = key index), the tile
// kernel's per-entry occurrence counts ecnt. Each key's count (its entries' counts,
// saturated to a byte) goes into the partitioned sketch (countmin.cuh: this workgroup owns
// every region its keys map to), then after a barrier every key is queried. Out: the kept
// keys at uo[0..D') in their order (sorted stays sorted), the kept entries at
// po / jo[eout .. eout + E') with the new key indices, and w_ent = 0 at the filtered
// entries -- the minibatch as if the filtered keys were absent, so the step, pack and
// owner kernels need no change. (D', E') -> res[0..1] (LDS).
__device__ __forceinline__ void tpf_filter_unit(uint64_t* __restrict__ uo, int32_t* __restrict__ po,
                                                uint16_t* __restrict__ jo, uint32_t D, uint32_t E,
                                                uint32_t ein, uint32_t eout,
                                                const uint8_t* __restrict__ ecnt, const CmArgs& cm,
                                                float* __restrict__ w_ent, int64_t w_cap,
                                                uint32_t* occ_big, uint32_t* occ_small,
                                                uint32_t* wkey, uint32_t* wval, uint32_t* lds,
                                                uint32_t* res, bool packed) {
  using namespace tp;
  constexpr int kKP = tpf::kUnitK / kBkThr;  // 4 keys per thread (contiguous)
  constexpr int kEP = 4;                      // entries per thread per chunk
  constexpr uint32_t kNone = 0xffffffffu;
  const int t = threadIdx.x;
  // the sketch words of the unit staged in LDS (block-uniform choice): <= kFlD keys
  const bool staged = D <= (uint32_t)kFlD && cm.k == kCmBatchK && cm.ncells32;
  uint32_t* occ = staged ? occ_small : occ_big;
  if (staged)
    for (uint32_t s = t; s < (uint32_t)kFlTab; s += kBkThr) wkey[s] = 0u;
  if (!packed)
    for (uint32_t j = t; j < D; j += kBkThr) occ[j] = 0u;
  __syncthreads();
  CmStage st;
  const bool stage = staged && D > 0;
  if (stage) cm_stage_begin(uo, D, cm, wkey, st, packed ? occ : nullptr);
  // occurrences per key: from the keys' top byte (packed: the LDS build summed them), or
  // 4 entries per thread per round, every load of a round in flight (clamped addresses,
  // selects afterwards)
  if (packed && !stage) {
    for (uint32_t j = t; j < D; j += kBkThr) occ[j] = (uint32_t)(uo[j] >> 56);
  }
  for (uint32_t c0 = 0; c0 < (packed ? 0u : E); c0 += kBkThr * 4) {
    uint32_t gi[4], jj[4], ec[4];
    int32_t id[4];
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      const uint32_t g = c0 + q * kBkThr + t;
      gi[q] = ein + (g < E ? g : E - 1);
      id[q] = po[gi[q]];
      jj[q] = jo[gi[q]];
    }
#pragma unroll
    for (int q = 0; q < 4; ++q) ec[q] = ecnt[id[q]];
#pragma unroll
    for (int q = 0; q < 4; ++q)
      if (c0 + q * kBkThr + t < E) atomicAdd(&occ[jj[q]], ec[q]);
  }
  __syncthreads();
  if (stage) {
    cm_stage_end(cm, occ, wval, st);
  } else if (D > 0 && !staged) {
    tpf_filter_global(uo, D, cm, occ);
  }
  __syncthreads();
  uint64_t key[kKP];
  uint32_t keep = 0, kc = 0;
#pragma unroll
  for (int q = 0; q < kKP; ++q) {  // contiguous keys per thread for the compaction
    const uint32_t j = t * kKP + q;
    key[q] = j < D ? uo[j] & kUoKey : 0ull;
    if (j < D && occ[j]) {
      keep |= 1u << q;
      ++kc;
    }
  }
  uint32_t Dn;
  uint32_t off = tp_block_scan<kBkThr>(kc, lds, &Dn);  // (barriers: every uo read is done)
#pragma unroll
  for (int q = 0; q < kKP; ++q) {
    const uint32_t j = t * kKP + q;
    if (j < D) {
      const bool k = (keep >> q) & 1u;
      occ[j] = k ? off : kNone;
      if (k) uo[off++] = key[q];
    }
  }
  __syncthreads();
  uint32_t eo = 0;
  for (uint32_t c0 = 0; c0 < E; c0 += kBkThr * kEP) {
    int32_t id[kEP];
    uint32_t nj[kEP], ec = 0;
#pragma unroll
    for (int q = 0; q < kEP; ++q) {
      const uint32_t g = c0 + t * kEP + q;
      nj[q] = kNone;
      id[q] = 0;
      if (g < E) {
        id[q] = po[ein + g];
        nj[q] = occ[jo[ein + g]];
        if (nj[q] != kNone) ++ec;
        else if (in_range(id[q], w_cap)) w_ent[id[q]] = 0.f;
      }
    }
    uint32_t tot;
    uint32_t o = eout + eo + tp_block_scan<kBkThr>(ec, lds, &tot);  // (reads done: barrier)
#pragma unroll
    for (int q = 0; q < kEP; ++q)
      if (nj[q] != kNone) {  // (output positions <= input ones: compaction)
        po[o] = id[q];
        jo[o] = (uint16_t)nj[q];
        ++o;
      }
    eo += tot;
  }
  if (t == 0) {
    res[0] = Dn;
    res[1] = eo;
  }
  __syncthreads();
}

// The fused tail filter of every bucket workgroup's units (tpf_filter_unit), one
// workgroup per bucket group, after tpf_bucket_kernel<true>: the partitioned CountMin
// insert + query of the minibatch's keys and the compaction of the filtered ones. A launch
// of its own so that only the sketch traffic runs in minibatch order (the callers chain
// these launches across their preparation streams; the bucket builds overlap freely):
// ordering the whole bucket kernel cost the pipelined step ~6.5 us
// (profiles/r6_tail_filter.log). cnt_pre <- the unfiltered counts, cnt <- the kept ones.
__global__ void __launch_bounds__(tp::kBkThr, 8)
tpf_filter_kernel(uint64_t* __restrict__ uniqf, int32_t* __restrict__ ent_pos,
                  uint16_t* __restrict__ ent_j, int32_t* __restrict__ cnt,
                  const uint8_t* __restrict__ ecnt, CmArgs cm, float* __restrict__ w_ent,
                  int64_t w_cap, int32_t* __restrict__ cnt_pre) {
  using namespace tp;
  __shared__ uint64_t hs[kDH];          // occ_big / the sketch table's values
  __shared__ uint64_t dl[kDH];          // the sketch table's word ids
  __shared__ uint32_t occs[kFlD];       // occ_small
  __shared__ uint32_t lds[kBkThr / 64 + 3];
  static_assert(kFlTab * 4 <= kDH * 8, "filter LDS");
  const int t = threadIdx.x, b = blockIdx.x;  // (tpf_xcd_group_of: measured and not kept)
  uint64_t* uo = uniqf + (int64_t)b * tpf::kUC;
  int32_t* po = ent_pos + (int64_t)b * tpf::kEC;
  uint16_t* jo = ent_j + (int64_t)b * tpf::kEC;
  int32_t* co = cnt + (int64_t)b * 4;
  const uint32_t D0 = (uint32_t)co[0], E0 = (uint32_t)co[1];
  const uint32_t D1 = (uint32_t)co[2], E1 = (uint32_t)co[3];
  // a unit the LDS build wrote carries its keys' counts in the top byte (every count >= 1);
  // the register-light units do not (their counts come from the entries)
  const bool packed = D0 > 0 && (uo[0] >> 56) != 0;
  uint32_t* occ = reinterpret_cast<uint32_t*>(hs);
  uint32_t* wkey = reinterpret_cast<uint32_t*>(dl);
  uint32_t* res = lds + kBkThr / 64 + 1;
  tpf_filter_unit(uo, po, jo, D0, E0, 0u, 0u, ecnt, cm, w_ent, w_cap, occ, occs, wkey, occ, lds,
                  res, packed);
  const uint32_t D0k = res[0], E0k = res[1];
  uint32_t D1k = 0, E1k = 0;
  if (D1 | E1) {
    __syncthreads();
    tpf_filter_unit(uo + tpf::kUnitK, po, jo, D1, E1, E0, E0k, ecnt, cm, w_ent, w_cap, occ, occs,
                    wkey, occ, lds, res, false);
    D1k = res[0];
    E1k = res[1];
  }
  if (t == 0) {
    if (cnt_pre) {  // the unfiltered counts (the exchange rows are sized from them)
      int32_t* cp = cnt_pre + (int64_t)b * 4;
      cp[0] = (int32_t)D0;
      cp[1] = (int32_t)E0;
      cp[2] = (int32_t)D1;
      cp[3] = (int32_t)E1;
    }
    co[0] = (int32_t)D0k;
    co[1] = (int32_t)E0k;
    co[2] = (int32_t)D1k;
    co[3] = (int32_t)E1k;
  }
}

// uniqf >= groups * kUC, ent_pos / ent_j >= groups * kEC, cnt >= groups * 4 (the host
// checks; tpf_groups)
// Tail filter (filt != null): ecnt >= tpf_stride_max(n) bytes, w_ent >= w_cap floats, and
// the sketch's regions no coarser than a fine bucket (region = key >> rshift, rshift <=
// shift; the host checks).
void localize_tpf(const uint64_t* raw, int64_t n, KeyMix m, void* temp, size_t temp_bytes,
                  int32_t* dcnt, uint16_t* rep, uint64_t* uniqf, int32_t* ent_pos, uint16_t* ent_j,
                  int32_t* cnt, int32_t* err, bool sorted, hipStream_t st, const CmArgs* filt,
                  uint8_t* ecnt, float* w_ent, int64_t w_cap, int32_t* cnt_pre, int stage) {
  if (n <= 0) return;
  if (!tploc_supported(n, m.bits)) throw std::runtime_error("localize_tpf: unsupported size");
  if (temp_bytes < tpf_temp_bytes(n, m.bits)) throw std::runtime_error("localize_tpf: temp");
  const TpGeom g = tp_geom(n, m.bits, true);
  if (filt && (filt->rshift > g.shift || !ecnt || !w_ent))
    throw std::runtime_error("localize_tpf: tail filter regions coarser than a bucket");
  char* p = (char*)temp;
  auto take = [&](size_t bytes) { char* r = p; p += al16(bytes); return r; };
  uint32_t* tkeys = (uint32_t*)take((size_t)g.N * 4);
  uint16_t* toff = (uint16_t*)take((size_t)g.T * (g.nbk + 1) * 2);
  // stage 1: the tile kernel only, 2: the bucket kernel only, 3: (tail filter) the filter
  // kernel only, 4: tile + bucket -- a caller orders something between them (the tail
  // filter's filter kernels run in minibatch order); 0: all
  const bool do_tile = stage != 2 && stage != 3;
  const bool do_bucket = stage != 1 && stage != 3;
  const bool do_filter = filt && stage != 1 && stage != 2 && stage != 4;
  // (the per-entry occurrence counts are written and read only with a tail filter)
  uint8_t* const ec = filt ? ecnt : nullptr;
  if (do_tile) tp_launch_tile(raw, n, m, g, tkeys, toff, dcnt, rep, err, ec, st);
  if (do_bucket) tpf_launch_bucket(g, tkeys, toff, uniqf, ent_pos, ent_j, cnt, err, sorted, ec, st);
  if (do_filter) {
    tpf_filter_kernel<<<(unsigned)tpf_groups_of(g), tp::kBkThr, 0, st>>>(
        uniqf, ent_pos, ent_j, cnt, ecnt, *filt, w_ent, w_cap, cnt_pre);
    PSAMD_HIP_CHECK(hipGetLastError());
  }
}

}  // namespace psamd
