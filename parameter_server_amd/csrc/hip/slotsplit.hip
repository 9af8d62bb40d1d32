// One parsed chunk (CSR row_ptr / keys / vals plus the feature group of every entry, as
// pstext.hip leaves them) split by feature group on the device (gfx950): slot-major keys /
// vals and one row-offset array per group, SlotData.from_batch's result. A strict fast path
// in the shape of textparse.hip / pstext.hip: separate launches, no hand-off between
// workgroups, and whatever is not certain leaves the chunk to the host (slotsplit.h).
//
//   1. ss_ids      a workgroup deduplicates the group ids of its tile of kSsTile features in
//                  an LDS table (only entries whose predecessor has another id insert) and
//                  adds its distinct ids to a global open-addressing table: a plain look-up,
//                  a CAS only where the id is missing.
//   2. ss_sort     one workgroup: bitonic sort of the table in LDS -> ids[S] ascending, S,
//                  the id and cell-cap checks, the cell count S * R.
//   3. ss_zero     start[S * R] = 0.
//   4. ss_runs     one thread per feature: row (a search of row_ptr between the rows of the
//                  tile's ends), group index (a search of ids in LDS), cell = index * R + row.
//                  The head of a (row, group) run exchanges its position + 1 into start[cell]
//                  -- a non-zero old value is a second run of that group in the row: defer --
//                  and the tail stores its position + 1 into end[cell].
//   5. ss_scan*    counts end - start per cell, exclusive scan over the cells in slot-major
//                  order (block sums, one workgroup over the sums, positions written over
//                  `end`): pos[cell] is where the cell's run goes and every group's row
//                  offsets at once.
//   6. ss_totals   the groups' entry counts into the header; ss_scatter moves feature i to
//                  pos[cell] + (i - (start[cell] - 1)).
//   7. ss_offsets  (after the header came back and S is known on the host) off[s][r].
// The only global atomics are ss_ids' inserts, ss_runs' head exchanges and the flag bits of
// a chunk that is handed back.
//
// Safety on arbitrary arrays: every index a kernel derives from the data (row, group index,
// cell, destination) is checked against its array before it is used; what does not fit
// sets kSsInput and the chunk is handed back. Every search loop is bounded.
#include "slotsplit.h"
#include "textparse.cuh"

#include <stdexcept>

namespace psamd {

namespace {

constexpr int kSsTile = 1024;  // features per workgroup (ss_ids, ss_runs, ss_scatter)
constexpr int kSsBlk = 256;    // threads of those workgroups
constexpr int kSsPer = kSsTile / kSsBlk;
constexpr int kSsMaxIds = 4096;
constexpr int kSsTab = 8192;   // global id table (a power of two, 2 x kSsMaxIds)
constexpr int kSsLds = 2048;   // a tile's id table in LDS (2 x kSsTile: never full)
constexpr int kSsScan = 4;     // cells per thread of the scan kernels
constexpr int kSsScanTile = kTpBlk * kSsScan;
constexpr uint32_t kSsEmpty = 0xffffffffu;
constexpr int64_t kSsDefaultCells = (int64_t)1 << 24;
constexpr int64_t kSsHdrWords = SS_IDS + 2 * kSsMaxIds;

__device__ __forceinline__ uint32_t ss_hash(uint32_t v) { return v * 2654435761u; }

__global__ void __launch_bounds__(kSsBlk) ss_ids_kernel(const int32_t* __restrict__ slots,
                                                        int64_t n, uint32_t* __restrict__ table,
                                                        int32_t* __restrict__ hdr) {
  __shared__ uint32_t lt[kSsLds];
  for (int k = threadIdx.x; k < kSsLds; k += kSsBlk) lt[k] = kSsEmpty;
  __syncthreads();
  const int64_t base = (int64_t)blockIdx.x * kSsTile;
  int outside = 0;
#pragma unroll
  for (int q = 0; q < kSsPer; ++q) {
    const int64_t i = base + q * kSsBlk + threadIdx.x;
    if (i >= n) continue;
    const int32_t v = slots[i];
    if (v < 0) {
      outside = 1;
      continue;
    }
    if (i != base && slots[i - 1] == v) continue;  // (its predecessor inserts)
    uint32_t h = (ss_hash((uint32_t)v) >> 21) & (kSsLds - 1);
    for (int p = 0; p < kSsLds; ++p) {
      const uint32_t old = atomicCAS(&lt[h], kSsEmpty, (uint32_t)v);
      if (old == kSsEmpty || old == (uint32_t)v) break;
      h = (h + 1) & (kSsLds - 1);
    }
  }
  __syncthreads();
  int full = 0;
  for (int k = threadIdx.x; k < kSsLds; k += kSsBlk) {
    const uint32_t v = lt[k];
    if (v == kSsEmpty) continue;
    uint32_t h = (ss_hash(v) >> 19) & (kSsTab - 1);
    bool done = false;
    for (int p = 0; p < kSsTab && !done; ++p) {
      uint32_t cur = __atomic_load_n(&table[h], __ATOMIC_RELAXED);
      if (cur == kSsEmpty) cur = atomicCAS(&table[h], kSsEmpty, v);
      done = cur == v || cur == kSsEmpty;
      h = (h + 1) & (kSsTab - 1);
    }
    if (!done) full = 1;  // (more than kSsTab ids)
  }
  if (outside | full) atomicOr(&hdr[SS_FLAGS], kSsIds);
}

// One workgroup: the table sorted in LDS (empty entries last), ids and S into the header.
__global__ void __launch_bounds__(kTpBlk) ss_sort_kernel(const uint32_t* __restrict__ table,
                                                         int64_t R, int64_t cell_cap,
                                                         int32_t* __restrict__ hdr) {
  __shared__ uint32_t a[kSsTab];
  __shared__ int s_count;
  for (int k = threadIdx.x; k < kSsTab; k += kTpBlk) a[k] = table[k];
  if (threadIdx.x == 0) s_count = 0;
  __syncthreads();
  for (int k = 2; k <= kSsTab; k <<= 1) {
    for (int j = k >> 1; j > 0; j >>= 1) {
      for (int t = threadIdx.x; t < kSsTab / 2; t += kTpBlk) {
        const int lo = ((t & ~(j - 1)) << 1) | (t & (j - 1)), hi = lo | j;
        const uint32_t x = a[lo], y = a[hi];
        if ((x > y) == ((lo & k) == 0)) {
          a[lo] = y;
          a[hi] = x;
        }
      }
      __syncthreads();
    }
  }
  for (int k = threadIdx.x; k < kSsTab; k += kTpBlk)
    if (a[k] != kSsEmpty && (k + 1 == kSsTab || a[k + 1] == kSsEmpty)) s_count = k + 1;
  __syncthreads();
  const int S = s_count;
  for (int k = threadIdx.x; k < kSsMaxIds; k += kTpBlk) hdr[SS_IDS + k] = k < S ? (int32_t)a[k] : 0;
  if (threadIdx.x == 0) {
    int flags = hdr[SS_FLAGS];
    if (S > kSsMaxIds) flags |= kSsIds;
    else if ((int64_t)S * (R + 1) > cell_cap) flags |= kSsCells;
    hdr[SS_FLAGS] = flags;
    hdr[SS_S] = S;
    hdr[SS_NCELLS] = flags ? 0 : (int32_t)((int64_t)S * R);
  }
}

__global__ void __launch_bounds__(256) ss_zero_kernel(int32_t* __restrict__ start,
                                                      const int32_t* __restrict__ hdr) {
  const int64_t nc = hdr[SS_NCELLS];
  for (int64_t c = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; c < nc;
       c += (int64_t)gridDim.x * blockDim.x)
    start[c] = 0;
}

// The row of entry p (row_ptr's own numbering) among rows [lo, hi]: the last r with
// row_ptr[r] <= p (rows without entries are skipped).
__device__ __forceinline__ int64_t ss_row_of(const int64_t* __restrict__ row_ptr, int64_t lo,
                                             int64_t hi, int64_t p) {
  for (int it = 0; it < 64 && lo < hi; ++it) {
    const int64_t mid = lo + (hi - lo + 1) / 2;
    if (row_ptr[mid] <= p) lo = mid;
    else hi = mid - 1;
  }
  return lo;
}

__global__ void __launch_bounds__(kSsBlk) ss_runs_kernel(
    const int64_t* __restrict__ row_ptr, int64_t R, const int32_t* __restrict__ slots, int64_t n,
    int32_t* __restrict__ start, int32_t* __restrict__ end, int32_t* __restrict__ cell,
    int32_t* __restrict__ hdr) {
  __shared__ int32_t ids[kSsMaxIds];
  __shared__ int64_t rng[2];
  // (the bits earlier launches set: the same in every thread; kSsRepeat / kSsInput may be
  // set while this kernel runs and are not looked at here)
  if (hdr[SS_FLAGS] & (kSsIds | kSsCells)) return;
  const int S = min(max(hdr[SS_S], 0), kSsMaxIds);
  const int64_t ncells = hdr[SS_NCELLS];
  for (int k = threadIdx.x; k < S; k += kSsBlk) ids[k] = hdr[SS_IDS + k];
  const int64_t base = (int64_t)blockIdx.x * kSsTile, p0 = row_ptr[0];
  const int64_t last = (base + kSsTile < n ? base + kSsTile : n) - 1;
  if (threadIdx.x < 2) rng[threadIdx.x] = ss_row_of(row_ptr, 0, R - 1, p0 + (threadIdx.x ? last : base));
  __syncthreads();
  const int64_t rlo = rng[0], rhi = rng[1] < rlo ? rlo : rng[1];
  int bad = 0, repeat = 0;
#pragma unroll
  for (int q = 0; q < kSsPer; ++q) {
    const int64_t i = base + q * kSsBlk + threadIdx.x;
    if (i >= n) continue;
    const int64_t r = ss_row_of(row_ptr, rlo, rhi, p0 + i);
    const int64_t rs = row_ptr[r] - p0, re = row_ptr[r + 1] - p0;
    const int32_t v = slots[i];
    int lo = 0, hi = S;  // lower bound of v in ids
    for (int it = 0; it < 13 && lo < hi; ++it) {
      const int mid = (lo + hi) >> 1;
      if (ids[mid] < v) lo = mid + 1;
      else hi = mid;
    }
    const int64_t c = (int64_t)lo * R + r;
    if (lo >= S || ids[lo] != v || i < rs || i >= re || re > n || !in_range(c, ncells)) {
      bad = 1;
      continue;
    }
    cell[i] = (int32_t)c;
    if (i == rs || slots[i - 1] != v)
      if (atomicExch(&start[c], (int32_t)(i + 1)) != 0) repeat = 1;
    if (i + 1 == re || slots[i + 1] != v) end[c] = (int32_t)(i + 1);
  }
  if (bad | repeat) atomicOr(&hdr[SS_FLAGS], (bad ? kSsInput : 0) | (repeat ? kSsRepeat : 0));
}

// entries of cell c: end - start where a run started there
__device__ __forceinline__ uint32_t ss_count(const int32_t* __restrict__ start,
                                             const int32_t* __restrict__ end, int64_t c,
                                             int64_t ncells, int64_t n) {
  if (c >= ncells) return 0u;
  const int64_t s = start[c];
  if (s <= 0) return 0u;
  const int64_t d = (int64_t)end[c] - s + 1;
  return d > 0 && d <= n ? (uint32_t)d : 0u;
}

// kWrite false: the tile's count into bsum; true: the positions over `end`, from the
// tile's base in bsum.
template <bool kWrite>
__global__ void __launch_bounds__(kTpBlk) ss_scan_kernel(const int32_t* __restrict__ start,
                                                         int32_t* __restrict__ end,
                                                         int32_t* __restrict__ bsum, int64_t n,
                                                         const int32_t* __restrict__ hdr) {
  __shared__ uint32_t lds_scan[kTpWaves + 1];
  const int64_t ncells = hdr[SS_FLAGS] ? 0 : hdr[SS_NCELLS];
  const int64_t c0 = (int64_t)blockIdx.x * kSsScanTile + (int64_t)threadIdx.x * kSsScan;
  if ((int64_t)blockIdx.x * kSsScanTile >= ncells) return;  // (the whole workgroup)
  uint32_t cnt[kSsScan], sum = 0;
#pragma unroll
  for (int q = 0; q < kSsScan; ++q) {
    cnt[q] = ss_count(start, end, c0 + q, ncells, n);
    sum += cnt[q];
  }
  uint32_t total;
  uint32_t ex = tp_block_scan<Sum>(sum, lds_scan, &total);
  if (!kWrite) {
    if (threadIdx.x == 0) bsum[blockIdx.x] = (int32_t)total;
    return;
  }
  ex += (uint32_t)bsum[blockIdx.x];
#pragma unroll
  for (int q = 0; q < kSsScan; ++q) {
    if (c0 + q < ncells) end[c0 + q] = (int32_t)ex;
    ex += cnt[q];
  }
}

// One workgroup: the tiles' counts -> their exclusive bases, in place; the grand total.
__global__ void __launch_bounds__(kTpBlk) ss_scan_sums_kernel(int32_t* __restrict__ bsum,
                                                              int64_t n,
                                                              int32_t* __restrict__ hdr) {
  __shared__ uint32_t lds_scan[kTpWaves + 1];
  const int64_t ncells = hdr[SS_FLAGS] ? 0 : hdr[SS_NCELLS];
  const int64_t nb = (ncells + kSsScanTile - 1) / kSsScanTile;
  uint32_t run = 0;
  for (int64_t b0 = 0; b0 < nb; b0 += kTpBlk) {
    const int64_t b = b0 + threadIdx.x;
    uint32_t total;
    const uint32_t ex = tp_block_scan<Sum>(b < nb ? (uint32_t)bsum[b] : 0u, lds_scan, &total);
    if (b < nb) bsum[b] = (int32_t)(run + ex);
    run += total;
  }
  if (threadIdx.x == 0) {
    hdr[SS_TOTAL] = (int32_t)run;
    if (!hdr[SS_FLAGS] && (int64_t)run != n) hdr[SS_FLAGS] = kSsInput;  // (an entry in no run)
  }
}

__global__ void __launch_bounds__(256) ss_totals_kernel(const int32_t* __restrict__ pos, int64_t R,
                                                        int32_t* __restrict__ hdr) {
  if (hdr[SS_FLAGS]) return;
  const int S = min(max(hdr[SS_S], 0), kSsMaxIds);
  const int64_t ncells = hdr[SS_NCELLS];
  for (int s = threadIdx.x; s < S; s += blockDim.x) {
    const int64_t a = (int64_t)s * R, b = a + R;
    if (!in_range(a, ncells)) continue;
    hdr[SS_IDS + kSsMaxIds + s] = (b < ncells ? pos[b] : hdr[SS_TOTAL]) - pos[a];
  }
}

template <bool kValued>
__global__ void __launch_bounds__(kSsBlk) ss_scatter_kernel(
    const uint64_t* __restrict__ keys, const float* __restrict__ vals,
    const int32_t* __restrict__ cell, const int32_t* __restrict__ start,
    const int32_t* __restrict__ pos, int64_t n, uint64_t* __restrict__ keys_out,
    float* __restrict__ vals_out, int32_t* __restrict__ hdr) {
  if (hdr[SS_FLAGS]) return;  // (set before this launch)
  const int64_t ncells = hdr[SS_NCELLS];
  const int64_t base = (int64_t)blockIdx.x * kSsTile;
#pragma unroll
  for (int q = 0; q < kSsPer; ++q) {
    const int64_t i = base + q * kSsBlk + threadIdx.x;
    if (i >= n) continue;
    const int64_t c = cell[i];
    if (!in_range(c, ncells)) continue;
    const int64_t d = (int64_t)pos[c] + (i - ((int64_t)start[c] - 1));
    if (!in_range(d, n)) continue;
    keys_out[d] = keys[i];
    if (kValued) vals_out[d] = vals[i];
  }
}

__global__ void __launch_bounds__(256) ss_offsets_kernel(const int32_t* __restrict__ pos, int64_t R,
                                                         int64_t S, int64_t n,
                                                         int64_t* __restrict__ off) {
  const int64_t ne = S * (R + 1), ncells = S * R;
  for (int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; e < ne;
       e += (int64_t)gridDim.x * blockDim.x) {
    const int64_t s = e / (R + 1), r = e - s * (R + 1);
    const int64_t c = s * R + r;  // (r == R: the next group's first cell)
    off[e] = (int64_t)(c < ncells ? pos[c] : (int32_t)n) - pos[s * R];
  }
}

struct SsWork {
  uint32_t* table;
  int32_t *bsum, *start, *pos, *cell;
  int64_t words;
};
inline SsWork ss_layout(int32_t* work, int64_t nnz, int64_t cells) {
  SsWork w;
  const int64_t nb = (cells + kSsScanTile - 1) / kSsScanTile + 1;
  w.table = reinterpret_cast<uint32_t*>(work);
  w.bsum = work + kSsTab;
  w.start = w.bsum + nb;
  w.pos = w.start + cells;
  w.cell = w.pos + cells;
  w.words = kSsTab + nb + 2 * cells + nnz;
  return w;
}
inline void ss_check_sizes(int64_t R, int64_t nnz, int64_t cells) {
  if (R < 1 || nnz < 1 || nnz >= ((int64_t)1 << 31) || R >= ((int64_t)1 << 31))
    throw std::invalid_argument("slotsplit: 1 <= rows, 1 <= nnz < 2^31");
  if (cells < 1 || cells > ((int64_t)1 << 30))
    throw std::invalid_argument("slotsplit: 1 <= cells <= 2^30");
}

}  // namespace

int slotsplit_tile() { return kSsTile; }
int slotsplit_max_ids() { return kSsMaxIds; }
int64_t slotsplit_default_cell_cap() { return kSsDefaultCells; }
int64_t slotsplit_hdr_words() { return kSsHdrWords; }
int64_t slotsplit_work_words(int64_t nnz, int64_t cells) {
  return ss_layout(nullptr, nnz, cells).words;
}

void slotsplit(const int64_t* row_ptr, int64_t R, const uint64_t* keys, const float* vals,
               const int32_t* slots, int64_t nnz, int64_t cell_cap, int64_t cells,
               uint64_t* keys_out, float* vals_out, int32_t* hdr, int32_t* work, hipStream_t st) {
  ss_check_sizes(R, nnz, cells);
  if (cell_cap < 0 || cell_cap > cells)
    throw std::invalid_argument("slotsplit: the cell cap must fit the work space's cells");
  if ((vals == nullptr) != (vals_out == nullptr))
    throw std::invalid_argument("slotsplit: vals and vals_out go together");
  const SsWork w = ss_layout(work, nnz, cells);
  const unsigned tiles = (unsigned)((nnz + kSsTile - 1) / kSsTile);
  const unsigned stiles = (unsigned)((cells + kSsScanTile - 1) / kSsScanTile);
  PSAMD_HIP_CHECK(hipMemsetAsync(hdr, 0, SS_IDS * sizeof(int32_t), st));
  PSAMD_HIP_CHECK(hipMemsetAsync(w.table, 0xff, kSsTab * sizeof(uint32_t), st));
  ss_ids_kernel<<<tiles, kSsBlk, 0, st>>>(slots, nnz, w.table, hdr);
  ss_sort_kernel<<<1, kTpBlk, 0, st>>>(w.table, R, cell_cap, hdr);
  ss_zero_kernel<<<grid_for(cells, 256, 2048), 256, 0, st>>>(w.start, hdr);
  ss_runs_kernel<<<tiles, kSsBlk, 0, st>>>(row_ptr, R, slots, nnz, w.start, w.pos, w.cell, hdr);
  ss_scan_kernel<false><<<stiles, kTpBlk, 0, st>>>(w.start, w.pos, w.bsum, nnz, hdr);
  ss_scan_sums_kernel<<<1, kTpBlk, 0, st>>>(w.bsum, nnz, hdr);
  ss_scan_kernel<true><<<stiles, kTpBlk, 0, st>>>(w.start, w.pos, w.bsum, nnz, hdr);
  ss_totals_kernel<<<1, 256, 0, st>>>(w.pos, R, hdr);
  if (vals)
    ss_scatter_kernel<true><<<tiles, kSsBlk, 0, st>>>(keys, vals, w.cell, w.start, w.pos, nnz,
                                                     keys_out, vals_out, hdr);
  else
    ss_scatter_kernel<false><<<tiles, kSsBlk, 0, st>>>(keys, vals, w.cell, w.start, w.pos, nnz,
                                                      keys_out, vals_out, hdr);
  PSAMD_HIP_CHECK(hipGetLastError());
}

void slotsplit_offsets(const int32_t* work, int64_t nnz, int64_t cells, int64_t R, int64_t S,
                       int64_t* off, hipStream_t st) {
  ss_check_sizes(R, nnz, cells);
  if (S < 1 || S > kSsMaxIds || S * (R + 1) > cells + S)
    throw std::invalid_argument("slotsplit_offsets: S groups of R rows outside the work space");
  const SsWork w = ss_layout(const_cast<int32_t*>(work), nnz, cells);
  ss_offsets_kernel<<<grid_for(S * (R + 1), 256, 4096), 256, 0, st>>>(w.pos, R, S, nnz, off);
  PSAMD_HIP_CHECK(hipGetLastError());
}

}  // namespace psamd
