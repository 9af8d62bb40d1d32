// Localisation fast path for key spaces of <= 32 bits (e.g. 10^9 hashed features).
//
// Stable LSD radix sort of (mixed u32 key, i32 position) with 8-bit digits:
//   pass 0 histogram kernel reads the RAW u64 keys, mixes them and writes the u32
//   mixed keys (so the separate mix pass disappears) and the positions are an
//   implicit iota (never read from memory in pass 0).
//   per pass: hist (LDS atomics) -> single-launch scan of the digit-major
//   histogram -> scatter.
// Scatter ranking is wave64-native: each wave owns 1024 consecutive tile
// elements, processed in 16 rounds of 64; lanes with equal digits are found with
// 8 __ballot()s (a 64-bit "match-any"), ranked with popcount, and a per-wave
// per-digit counter in LDS carries the rank across rounds. A 256-thread digit
// scan turns (digit, wave) counts into tile offsets; the tile is reordered in LDS
// and stored digit-run contiguous.
// RLE (unique keys, segment ids, local columns) is fused into 2 kernels + scan.
// All global indices are bounds-checked.
// Tried and measured (65,536 x 39 Criteo keys): one-sweep passes with per-digit
// decoupled look-back (1 global-histogram kernel + 3 scatter passes) were correct
// but 7.9 ms vs 0.2 ms: with ~600 tiles resident at once every tile walks the
// predecessors' published counts serially; the reduce-then-scan passes stay.
#include "sort32.h"
#include "common.cuh"

#include <algorithm>
#include <stdexcept>
#include <string>

namespace psamd {

namespace s32 {
constexpr int kBlk = 256;
constexpr int kWaves = kBlk / 64;
constexpr int kItems = 16;
constexpr int kTile = kBlk * kItems;  // 4096
constexpr int kMaxBits = 10;            // digit width: 8 (4 passes for 30-bit keys)
constexpr int kMaxDigits = 1 << kMaxBits;  // or 10 (3 passes), a template parameter
}  // namespace s32
using namespace s32;

__device__ __forceinline__ uint32_t block_excl_scan_u32(uint32_t v, uint32_t* lds, uint32_t* total,
                                                        int nwaves) {
  const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
  uint32_t x = v;
#pragma unroll
  for (int off = 1; off < 64; off <<= 1) {
    uint32_t y = __shfl_up(x, off, 64);
    if (lane >= off) x += y;
  }
  if (lane == 63) lds[wid] = x;
  __syncthreads();
  if (threadIdx.x == 0) {
    uint32_t run = 0;
    for (int w = 0; w < nwaves; ++w) {
      uint32_t t = lds[w];
      lds[w] = run;
      run += t;
    }
    lds[nwaves] = run;
  }
  __syncthreads();
  const uint32_t r = x - v + lds[wid];
  *total = lds[nwaves];
  __syncthreads();
  return r;
}

// Device-side element counts (n_dev): a launch sized for n_host keys only works
// on the first ceil(n/kTile) tiles; per-tile arrays (histogram columns, tile
// partials) use that live tile count as their stride, so later kernels and the
// scans never touch the unused tail. n_dev == nullptr: host n, as before.
__device__ __forceinline__ int64_t live_tiles(const int32_t* n_dev, int64_t n_host,
                                              int64_t T_host) {
  if (!n_dev) return T_host;
  return (dev_len(n_dev, n_host) + kTile - 1) / kTile;
}

// ---------------------------------------------------------------- histogram
template <bool kMix, int kBits>
__global__ void __launch_bounds__(kBlk)
hist32_kernel(const uint64_t* __restrict__ raw, const uint32_t* __restrict__ keys, int64_t n_host,
              KeyMix m, uint32_t* __restrict__ mixed_out, int shift, uint32_t* __restrict__ hist,
              int64_t T_host, const int32_t* __restrict__ n_dev,
              const int32_t* __restrict__ tile_cnt) {
  constexpr int kDigits = 1 << kBits;
  const int64_t n = dev_len(n_dev, n_host);
  const int64_t T = live_tiles(n_dev, n_host, T_host);
  if ((int64_t)blockIdx.x >= T) return;
  __shared__ uint32_t cnt[kDigits];
  for (int d = threadIdx.x; d < kDigits; d += kBlk) cnt[d] = 0;
  __syncthreads();
  const int64_t base = (int64_t)blockIdx.x * kTile;
  // ragged input (tile_cnt): tile b holds tile_cnt[b] keys at [b*kTile, ...)
  const int64_t lim = tile_cnt ? base + min(kTile, max(0, tile_cnt[blockIdx.x])) : n;
  if (!kMix && base + kTile <= lim) {
    // full tile: 16-byte loads, 4 keys per load, 4 loads per thread
    const uint4* kv = reinterpret_cast<const uint4*>(keys + base);
#pragma unroll
    for (int j = 0; j < kItems / 4; ++j) {
      const uint4 q = kv[j * kBlk + threadIdx.x];
      atomicAdd(&cnt[(q.x >> shift) & (kDigits - 1)], 1u);
      atomicAdd(&cnt[(q.y >> shift) & (kDigits - 1)], 1u);
      atomicAdd(&cnt[(q.z >> shift) & (kDigits - 1)], 1u);
      atomicAdd(&cnt[(q.w >> shift) & (kDigits - 1)], 1u);
    }
  } else {
#pragma unroll
    for (int j = 0; j < kItems; ++j) {
      const int64_t i = base + j * kBlk + threadIdx.x;
      if (i < lim) {
        uint32_t k;
        if (kMix) {
          k = (uint32_t)mix_key(raw[i], m);
          mixed_out[i] = k;
        } else {
          k = keys[i];
        }
        atomicAdd(&cnt[(k >> shift) & (kDigits - 1)], 1u);
      }
    }
  }
  __syncthreads();
  for (int d = threadIdx.x; d < kDigits; d += kBlk) hist[(int64_t)d * T + blockIdx.x] = cnt[d];
}

// ------------------------------------------------------------ 2-launch scan
// Exclusive scan of a[0:n] in place: (1) per-2048-chunk sums, (2) each chunk
// block sums the partials of all earlier chunks itself (few hundred L2-resident
// values), then scans its chunk. No single-block serial phase, no spinning.
constexpr int kScanChunk = 2048;

// n_dev: the scanned array holds live_tiles(n_dev) * per_tile entries.
__device__ __forceinline__ int64_t scan_len(int64_t n_host, const int32_t* n_dev, int64_t n_items,
                                            int64_t per_tile) {
  if (!n_dev) return n_host;
  const int64_t v = live_tiles(n_dev, n_items, 0) * per_tile;
  return v < n_host ? v : n_host;
}

__global__ void __launch_bounds__(kBlk) chunk_sum_kernel(const uint32_t* __restrict__ a,
                                                         int64_t n_host, uint32_t* __restrict__ part,
                                                         const int32_t* __restrict__ n_dev,
                                                         int64_t n_items, int64_t per_tile) {
  const int64_t n = scan_len(n_host, n_dev, n_items, per_tile);
  if ((int64_t)blockIdx.x * kScanChunk >= n) return;
  __shared__ uint32_t lds[kWaves + 1];
  const int64_t base = (int64_t)blockIdx.x * kScanChunk;
  uint32_t s = 0;
#pragma unroll
  for (int j = 0; j < kScanChunk / kBlk; ++j) {
    const int64_t i = base + j * kBlk + threadIdx.x;
    if (i < n) s += a[i];
  }
  uint32_t tot;
  block_excl_scan_u32(s, lds, &tot, kWaves);
  if (threadIdx.x == 0) part[blockIdx.x] = tot;
}

__global__ void __launch_bounds__(kBlk) chunk_scan_kernel(uint32_t* __restrict__ a, int64_t n_host,
                                                          const uint32_t* __restrict__ part,
                                                          const int32_t* __restrict__ n_dev,
                                                          int64_t n_items, int64_t per_tile) {
  const int64_t n = scan_len(n_host, n_dev, n_items, per_tile);
  if ((int64_t)blockIdx.x * kScanChunk >= n) return;
  __shared__ uint32_t tile[kScanChunk];
  __shared__ uint32_t lds[kWaves + 1];
  // prefix of earlier chunks
  uint32_t pre = 0;
  for (int64_t i = threadIdx.x; i < (int64_t)blockIdx.x; i += kBlk) pre += part[i];
  uint32_t tot;
  block_excl_scan_u32(pre, lds, &tot, kWaves);
  const uint32_t offset = tot;
  const int64_t base = (int64_t)blockIdx.x * kScanChunk;
  constexpr int kPer = kScanChunk / kBlk;  // 8
#pragma unroll
  for (int j = 0; j < kPer; ++j) {
    const int64_t i = base + j * kBlk + threadIdx.x;
    tile[j * kBlk + threadIdx.x] = i < n ? a[i] : 0u;
  }
  __syncthreads();
  uint32_t v[kPer], s = 0;
#pragma unroll
  for (int q = 0; q < kPer; ++q) { v[q] = tile[threadIdx.x * kPer + q]; s += v[q]; }
  uint32_t run = block_excl_scan_u32(s, lds, &tot, kWaves) + offset;
#pragma unroll
  for (int q = 0; q < kPer; ++q) { tile[threadIdx.x * kPer + q] = run; run += v[q]; }
  __syncthreads();
#pragma unroll
  for (int j = 0; j < kPer; ++j) {
    const int64_t i = base + j * kBlk + threadIdx.x;
    if (i < n) a[i] = tile[j * kBlk + threadIdx.x];
  }
}

void scan2_u32(uint32_t* a, int64_t n, uint32_t* part, hipStream_t st,
               const int32_t* n_dev = nullptr, int64_t n_items = 0, int64_t per_tile = 1) {
  const int64_t chunks = (n + kScanChunk - 1) / kScanChunk;
  chunk_sum_kernel<<<(unsigned)chunks, kBlk, 0, st>>>(a, n, part, n_dev, n_items, per_tile);
  PSAMD_HIP_CHECK(hipGetLastError());
  chunk_scan_kernel<<<(unsigned)chunks, kBlk, 0, st>>>(a, n, part, n_dev, n_items, per_tile);
  PSAMD_HIP_CHECK(hipGetLastError());
}

// ------------------------------------------------------------------ scatter
// kScatThreads threads per 4096-key tile: 16 waves x 256 keys (4 ranking rounds
// per wave instead of 16), per-wave digit counters as u16 and the tile's global
// digit offsets cached in LDS (68 KB -> 2 tiles per CU, 8 waves per SIMD).
constexpr int kScatThreads = 1024;

template <int kBits>
__global__ void __launch_bounds__(kScatThreads)
scatter32_kernel(const uint32_t* __restrict__ keys_in, const int32_t* __restrict__ vals_in,
                 uint32_t* __restrict__ keys_out, int32_t* __restrict__ vals_out, int64_t n_host,
                 int shift, const uint32_t* __restrict__ offs, int64_t T_host,
                 const int32_t* __restrict__ n_dev, const int32_t* __restrict__ tile_cnt) {
  constexpr int kDigits = 1 << kBits;
  constexpr int kT = kScatThreads;
  constexpr int kW = kT / 64;
  constexpr int kIt = kTile / kT;                       // keys per lane
  constexpr int kDPT = kDigits >= kT ? kDigits / kT : 1;  // digits per thread in the scan
  const int64_t n = dev_len(n_dev, n_host);
  const int64_t T = live_tiles(n_dev, n_host, T_host);
  if ((int64_t)blockIdx.x >= T) return;
  __shared__ uint32_t skeys[kTile];
  __shared__ int32_t svals[kTile];
  __shared__ uint16_t wcnt[kW * kDigits];  // [wave][digit]: counts, then tile offsets
  __shared__ int32_t goff[kDigits];        // global position of the tile's digit run - start
  __shared__ uint32_t lds[kW + 1];
  const int t = threadIdx.x, lane = t & 63, w = t >> 6;
  const int64_t base = (int64_t)blockIdx.x * kTile;
  const int tile_n = tile_cnt ? min(kTile, max(0, tile_cnt[blockIdx.x]))
                              : (int)min((int64_t)kTile, n - base);
  for (int f = t; f < kW * kDigits; f += kT) wcnt[f] = 0;
  __syncthreads();
  uint32_t k[kIt];
  int32_t v[kIt];
  uint32_t rank[kIt];
  const uint64_t lt_mask = (1ull << lane) - 1ull;
#pragma unroll
  for (int r = 0; r < kIt; ++r) {  // all loads in flight before the ranking chain
    const int li = w * (kTile / kW) + r * 64 + lane;  // wave-owned 256-key segment
    if (li < tile_n) {
      k[r] = keys_in[base + li];
      v[r] = vals_in ? vals_in[base + li] : (int32_t)(base + li);
    }
  }
#pragma unroll
  for (int r = 0; r < kIt; ++r) {
    const int li = w * (kTile / kW) + r * 64 + lane;
    const bool valid = li < tile_n;
    uint32_t d = kDigits;  // sentinel for invalid lanes
    if (valid) d = (k[r] >> shift) & (kDigits - 1);
    uint64_t peers = __ballot(valid);  // 64-lane match-any on the digit
#pragma unroll
    for (int b = 0; b < kBits; ++b) {
      const bool bit = (d >> b) & 1u;
      const uint64_t bal = __ballot(bit);
      peers &= bit ? bal : ~bal;
    }
    uint32_t base_cnt = 0;
    if (valid) base_cnt = wcnt[w * kDigits + d];
    __builtin_amdgcn_wave_barrier();
    if (valid && (peers & lt_mask) == 0ull)
      wcnt[w * kDigits + d] = (uint16_t)(base_cnt + (uint32_t)__popcll(peers));
    __builtin_amdgcn_wave_barrier();
    rank[r] = base_cnt + (uint32_t)__popcll(peers & lt_mask);
  }
  __syncthreads();
  {  // digit-major tile offsets; thread t owns digits [t*kDPT, (t+1)*kDPT)
    uint32_t tot_d[kDPT], s_t = 0;
#pragma unroll
    for (int e = 0; e < kDPT; ++e) {
      const int d = t * kDPT + e;
      uint32_t c = 0;
      if (d < kDigits) {
#pragma unroll
        for (int q = 0; q < kW; ++q) c += wcnt[q * kDigits + d];
      }
      tot_d[e] = c;
      s_t += c;
    }
    uint32_t total;
    uint32_t run = block_excl_scan_u32(s_t, lds, &total, kW);
#pragma unroll
    for (int e = 0; e < kDPT; ++e) {
      const int d = t * kDPT + e;
      if (d < kDigits) {
        goff[d] = (int32_t)offs[(int64_t)d * T + blockIdx.x] - (int32_t)run;
        uint32_t r2 = run;
#pragma unroll
        for (int q = 0; q < kW; ++q) {
          const uint32_t c = wcnt[q * kDigits + d];
          wcnt[q * kDigits + d] = (uint16_t)r2;
          r2 += c;
        }
      }
      run += tot_d[e];
    }
  }
  __syncthreads();
#pragma unroll
  for (int r = 0; r < kIt; ++r) {
    const int li = w * (kTile / kW) + r * 64 + lane;
    if (li < tile_n) {
      const uint32_t d = (k[r] >> shift) & (kDigits - 1);
      const uint32_t pos = wcnt[w * kDigits + d] + rank[r];
      if (pos < (uint32_t)kTile) {
        skeys[pos] = k[r];
        svals[pos] = v[r];
      }
    }
  }
  __syncthreads();
#pragma unroll
  for (int j = 0; j < kIt; ++j) {
    const int li = j * kT + t;
    if (li < tile_n) {
      const uint32_t key = skeys[li];
      const uint32_t d = (key >> shift) & (kDigits - 1);
      const int64_t g = (int64_t)goff[d] + li;
      if (in_range(g, n_host)) {
        keys_out[g] = key;
        vals_out[g] = svals[li];
      }
    }
  }
}

// -------------------------------------------------------------- fused RLE
__global__ void __launch_bounds__(kBlk) rle32_count_kernel(const uint32_t* __restrict__ hs,
                                                           int64_t n_host, uint32_t* __restrict__ part,
                                                           const int32_t* __restrict__ n_dev) {
  const int64_t n = dev_len(n_dev, n_host);
  if ((int64_t)blockIdx.x >= live_tiles(n_dev, n_host, (n_host + kTile - 1) / kTile)) return;
  __shared__ uint32_t lds[kWaves + 1];
  const int64_t base = (int64_t)blockIdx.x * kTile;
  uint32_t c = 0;
#pragma unroll 4
  for (int j = 0; j < kItems; ++j) {
    const int64_t i = base + j * kBlk + threadIdx.x;
    if (i < n) c += (i == 0 || hs[i] != hs[i - 1]) ? 1u : 0u;
  }
  uint32_t tot;
  block_excl_scan_u32(c, lds, &tot, kWaves);
  if (threadIdx.x == 0) part[blockIdx.x] = tot;
}

// part[] holds the exclusive prefix of head counts per tile (scan_single_kernel).
__global__ void __launch_bounds__(kBlk)
rle32_write_kernel(const uint32_t* __restrict__ hs, const int32_t* __restrict__ pos_s, int64_t n_host,
                   const uint32_t* __restrict__ part, int32_t* __restrict__ segid,
                   uint64_t* __restrict__ uniq, int32_t* __restrict__ seg_start,
                   int32_t* __restrict__ local_col, int32_t* __restrict__ n_uniq,
                   float* __restrict__ zero_a, float* __restrict__ zero_b,
                   const int32_t* __restrict__ n_dev, int64_t p_cap) {
  const int64_t n = dev_len(n_dev, n_host);
  if (n == 0 && blockIdx.x == 0 && threadIdx.x == 0) {
    *n_uniq = 0;
    seg_start[0] = 0;
  }
  if ((int64_t)blockIdx.x >= live_tiles(n_dev, n_host, (n_host + kTile - 1) / kTile)) return;
  // flag[] is read both coalesced (li = j*256 + t) and blocked (t*16 + q): pad one
  // word per 16 so the blocked pass does not put all 64 lanes on 2 LDS banks
  __shared__ uint32_t flag[kTile + kTile / 16 + 1];
  __shared__ uint32_t lds[kWaves + 1];
  const int t = threadIdx.x;
  const int64_t base = (int64_t)blockIdx.x * kTile;
  const int tile_n = (int)min((int64_t)kTile, n - base);
#pragma unroll
  for (int j = 0; j < kItems; ++j) {  // coalesced flag computation into LDS
    const int li = j * kBlk + t;
    const int64_t i = base + li;
    flag[li + (li >> 4)] = (li < tile_n) ? ((i == 0 || hs[i] != hs[i - 1]) ? 1u : 0u) : 0u;
  }
  __syncthreads();
  // blocked: thread t owns tile elements [t*16, t*16+16)
  uint32_t s = 0;
#pragma unroll
  for (int q = 0; q < kItems; ++q) s += flag[t * (kItems + 1) + q];
  uint32_t tot;
  uint32_t run = block_excl_scan_u32(s, lds, &tot, kWaves) + part[blockIdx.x];
#pragma unroll
  for (int q = 0; q < kItems; ++q) {
    run += flag[t * (kItems + 1) + q];
    flag[t * (kItems + 1) + q] = run;  // inclusive 1-based segment id
  }
  __syncthreads();
#pragma unroll 4
  for (int j = 0; j < kItems; ++j) {
    const int li = j * kBlk + t;
    if (li >= tile_n) continue;
    const int64_t i = base + li;
    const uint32_t sid = flag[li + (li >> 4)];
    const int32_t s0 = (int32_t)sid - 1;
    segid[i] = (int32_t)sid;
    if (!in_range(s0, n)) continue;
    const int32_t p = pos_s[i];
    if (in_range(p, p_cap)) local_col[p] = s0;
    const bool head = (i == 0) || hs[i] != hs[i - 1];
    if (head) {
      uniq[s0] = hs[i];
      seg_start[s0] = (int32_t)i;
      if (zero_a) zero_a[s0] = 0.f;
      if (zero_b) zero_b[s0] = 0.f;
    }
    if (i == n - 1) {
      *n_uniq = s0 + 1;
      seg_start[s0 + 1] = (int32_t)n;
    }
  }
}

// ---------------------------------------------------------------------------
// Workspace: [mixed keys n*4][keys tmp n*4][vals tmp n*4][hist D*T*4][part T*4][scan parts]
// (sized for the widest digit, D = 1024)
size_t localize32_temp_bytes(int64_t n) {
  const int64_t T = (n + kTile - 1) / kTile;
  const int64_t chunks = ((int64_t)kMaxDigits * T + kScanChunk - 1) / kScanChunk + T;
  return (size_t)n * 12 + (size_t)kMaxDigits * T * 4 + (size_t)T * 4 + (size_t)chunks * 4 + 512;
}

// keys (raw u64) -> hs (mixed u32 sorted), pos_s; then RLE outputs.
template <int kBits>
static void radix32(const uint64_t* raw, int64_t n, KeyMix m, int64_t T, uint32_t* mixed,
                    uint32_t* kt, int32_t* vt, uint32_t* hist, uint32_t* spart, uint32_t* hs,
                    int32_t* pos_s, hipStream_t st) {
  constexpr int kDigits = 1 << kBits;
  const int passes = (m.bits + kBits - 1) / kBits;
  const uint32_t* src_k = mixed;
  const int32_t* src_v = nullptr;  // iota
  for (int pass = 0; pass < passes; ++pass) {
    const bool to_out = ((passes - 1 - pass) % 2) == 0;
    uint32_t* dk = to_out ? hs : kt;
    int32_t* dv = to_out ? pos_s : vt;
    const int shift = pass * kBits;
    if (pass == 0)
      hist32_kernel<true, kBits><<<(unsigned)T, kBlk, 0, st>>>(raw, nullptr, n, m, mixed, shift,
                                                               hist, T, nullptr, nullptr);
    else
      hist32_kernel<false, kBits><<<(unsigned)T, kBlk, 0, st>>>(nullptr, src_k, n, m, nullptr,
                                                                shift, hist, T, nullptr, nullptr);
    PSAMD_HIP_CHECK(hipGetLastError());
    scan2_u32(hist, (int64_t)kDigits * T, spart, st);
    scatter32_kernel<kBits><<<(unsigned)T, kScatThreads, 0, st>>>(src_k, src_v, dk, dv, n, shift, hist, T,
                                                          nullptr, nullptr);
    PSAMD_HIP_CHECK(hipGetLastError());
    src_k = dk;
    src_v = dv;
  }
}

void localize32(const uint64_t* raw, int64_t n, KeyMix m, void* temp, size_t temp_bytes,
                uint32_t* hs, int32_t* pos_s, int32_t* segid, uint64_t* uniq, int32_t* seg_start,
                int32_t* local_col, int32_t* n_uniq, float* zero_a, float* zero_b, int digit_bits,
                hipStream_t st) {
  if (n <= 0) return;
  if (m.bits > 32) throw std::runtime_error("localize32 needs key bits <= 32");
  if (temp_bytes < localize32_temp_bytes(n)) throw std::runtime_error("localize32 temp too small");
  const int64_t T = (n + kTile - 1) / kTile;
  char* p = (char*)temp;
  uint32_t* mixed = (uint32_t*)p;
  p += (size_t)n * 4;
  uint32_t* kt = (uint32_t*)p;
  p += (size_t)n * 4;
  int32_t* vt = (int32_t*)p;
  p += (size_t)n * 4;
  uint32_t* hist = (uint32_t*)p;
  p += (size_t)kMaxDigits * T * 4;
  uint32_t* part = (uint32_t*)p;
  p += (size_t)T * 4;
  uint32_t* spart = (uint32_t*)p;  // chunk partials for scan2
  if (digit_bits == 10)
    radix32<10>(raw, n, m, T, mixed, kt, vt, hist, spart, hs, pos_s, st);
  else
    radix32<8>(raw, n, m, T, mixed, kt, vt, hist, spart, hs, pos_s, st);
  rle32_count_kernel<<<(unsigned)T, kBlk, 0, st>>>(hs, n, part, nullptr);
  PSAMD_HIP_CHECK(hipGetLastError());
  scan2_u32(part, T, spart, st);
  rle32_write_kernel<<<(unsigned)T, kBlk, 0, st>>>(hs, pos_s, n, part, segid, uniq, seg_start,
                                                   local_col, n_uniq, zero_a, zero_b, nullptr, n);
  PSAMD_HIP_CHECK(hipGetLastError());
}

// ---------------------------------------------------------------------------
// 33..40-bit key spaces (10^10 features: 34 bits) with n < 2^22 keys: the same
// 10-bit u32 passes, 4 of them instead of the generic u64 sort's 5 x 8-bit ones.
// The mixed key h splits into lo = h mod 2^30 (the u32 sort key) and hi = h >> 30
// (<= 10 bits), carried in the value next to the position: v = pos | hi << 22.
// Passes 0-2 sort (lo, v) by lo's three digits; pass 3 swaps the roles, key = v,
// value = lo, digit = v >> 22 = hi, so the stable result is ordered by (hi, lo) = h.
// The combine kernel writes the sorted u64 keys and positions for the u64 RLE.
constexpr int kPos40 = 22;

__global__ void __launch_bounds__(kBlk)
mix40_kernel(const uint64_t* __restrict__ raw, int64_t n, KeyMix m, uint32_t* __restrict__ lo,
             int32_t* __restrict__ v) {
  for (int64_t i = (int64_t)blockIdx.x * kBlk + threadIdx.x; i < n; i += (int64_t)gridDim.x * kBlk) {
    const uint64_t h = mix_key(raw[i], m);
    lo[i] = (uint32_t)(h & ((1u << 30) - 1));
    v[i] = (int32_t)((uint32_t)i | ((uint32_t)(h >> 30) << kPos40));
  }
}

__global__ void __launch_bounds__(kBlk)
combine40_kernel(const uint32_t* __restrict__ v, const int32_t* __restrict__ lo, int64_t n,
                 uint64_t* __restrict__ hs, int32_t* __restrict__ pos_s) {
  for (int64_t i = (int64_t)blockIdx.x * kBlk + threadIdx.x; i < n; i += (int64_t)gridDim.x * kBlk) {
    const uint32_t vi = v[i];
    hs[i] = ((uint64_t)(vi >> kPos40) << 30) | (uint64_t)(uint32_t)lo[i];
    pos_s[i] = (int32_t)(vi & ((1u << kPos40) - 1));
  }
}

size_t sort40_temp_bytes(int64_t n) {
  const int64_t T = (n + kTile - 1) / kTile;
  const int64_t chunks = ((int64_t)kMaxDigits * T + kScanChunk - 1) / kScanChunk + T;
  const int64_t na = (n + 3) & ~int64_t(3);  // 16-B aligned arrays (vector loads)
  return (size_t)na * 16 + (size_t)kMaxDigits * T * 4 + (size_t)chunks * 4 + 512;
}

void sort40(const uint64_t* raw, int64_t n, KeyMix m, void* temp, size_t temp_bytes,
            uint64_t* hs, int32_t* pos_s, hipStream_t st) {
  if (n <= 0) return;
  if (m.bits <= 30 || m.bits > 40) throw std::runtime_error("sort40 needs 30 < key bits <= 40");
  if (n >= (int64_t(1) << kPos40)) throw std::runtime_error("sort40 needs n < 2^22 keys");
  if (temp_bytes < sort40_temp_bytes(n)) throw std::runtime_error("sort40 temp too small");
  const int64_t T = (n + kTile - 1) / kTile;
  const int64_t na = (n + 3) & ~int64_t(3);
  char* p = (char*)temp;
  uint32_t* ak = (uint32_t*)p;
  p += (size_t)na * 4;
  int32_t* av = (int32_t*)p;
  p += (size_t)na * 4;
  uint32_t* bk = (uint32_t*)p;
  p += (size_t)na * 4;
  int32_t* bv = (int32_t*)p;
  p += (size_t)na * 4;
  uint32_t* hist = (uint32_t*)p;
  p += (size_t)kMaxDigits * T * 4;
  uint32_t* spart = (uint32_t*)p;
  const unsigned g = (unsigned)std::min<int64_t>((n + kBlk - 1) / kBlk, 4096);
  mix40_kernel<<<g, kBlk, 0, st>>>(raw, n, m, ak, av);
  PSAMD_HIP_CHECK(hipGetLastError());
  KeyMix none{};
  auto pass = [&](const uint32_t* sk, const int32_t* sv, uint32_t* dk, int32_t* dv, int shift) {
    hist32_kernel<false, 10><<<(unsigned)T, kBlk, 0, st>>>(nullptr, sk, n, none, nullptr, shift,
                                                           hist, T, nullptr, nullptr);
    PSAMD_HIP_CHECK(hipGetLastError());
    scan2_u32(hist, (int64_t)1024 * T, spart, st);
    scatter32_kernel<10><<<(unsigned)T, kScatThreads, 0, st>>>(sk, sv, dk, dv, n, shift, hist, T,
                                                              nullptr, nullptr);
    PSAMD_HIP_CHECK(hipGetLastError());
  };
  pass(ak, av, bk, bv, 0);
  pass(bk, bv, ak, av, 10);
  pass(ak, av, bk, bv, 20);
  // pass 3: key = v (digit hi = v >> 22), value = lo
  pass(reinterpret_cast<const uint32_t*>(bv), reinterpret_cast<const int32_t*>(bk), ak, av,
       kPos40);
  combine40_kernel<<<g, kBlk, 0, st>>>(ak, av, n, hs, pos_s);
  PSAMD_HIP_CHECK(hipGetLastError());
}

// ---------------------------------------------------------------------------
// Sort + RLE of already-mixed u32 keys held in ragged tiles (the output of the
// tile-deduplicating localiser, tileloc.hip): n_dev = total live keys, n_max the
// workspace. After the first pass every kernel, scan and tile stride follows the
// live count, so the cost scales with n_dev, not with n_max.
size_t sort32_dev_temp_bytes(int64_t n_max) {
  const int64_t T = (n_max + kTile - 1) / kTile;
  const int64_t chunks = ((int64_t)kMaxDigits * T + kScanChunk - 1) / kScanChunk + T;
  return (size_t)n_max * 8 + (size_t)kMaxDigits * T * 4 + (size_t)T * 4 + (size_t)chunks * 4 + 512;
}

// Pass 0 reads RAGGED tiles (tile b = tile_cnt[b] keys at [b*kTile, ...), values =
// the implicit fixed-stride ids b*kTile + i) and writes them compacted; later passes
// work on the n_dev compacted elements.
template <int kBits>
static void radix32_dev(const uint32_t* keys_in, const int32_t* tile_cnt, int64_t n, int64_t T,
                        const int32_t* n_dev, int bits, uint32_t* kt, int32_t* vt, uint32_t* hist,
                        uint32_t* spart, uint32_t* hs, int32_t* pos_s, hipStream_t st) {
  constexpr int kDigits = 1 << kBits;
  const int passes = (bits + kBits - 1) / kBits;
  const uint32_t* src_k = keys_in;
  const int32_t* src_v = nullptr;  // pass 0: fixed-stride ids (iota)
  KeyMix none{};
  for (int pass = 0; pass < passes; ++pass) {
    const bool to_out = ((passes - 1 - pass) % 2) == 0;
    uint32_t* dk = to_out ? hs : kt;
    int32_t* dv = to_out ? pos_s : vt;
    const int shift = pass * kBits;
    const int32_t* nd = pass == 0 ? nullptr : n_dev;
    const int32_t* tc = pass == 0 ? tile_cnt : nullptr;
    hist32_kernel<false, kBits><<<(unsigned)T, kBlk, 0, st>>>(nullptr, src_k, n, none, nullptr,
                                                              shift, hist, T, nd, tc);
    PSAMD_HIP_CHECK(hipGetLastError());
    scan2_u32(hist, (int64_t)kDigits * T, spart, st, nd, n, kDigits);
    scatter32_kernel<kBits><<<(unsigned)T, kScatThreads, 0, st>>>(src_k, src_v, dk, dv, n, shift, hist, T,
                                                          nd, tc);
    PSAMD_HIP_CHECK(hipGetLastError());
    src_k = dk;
    src_v = dv;
  }
}

void sort_rle32_dev(const uint32_t* keys_in, const int32_t* tile_cnt, int64_t n_max,
                    const int32_t* n_dev, int bits, int digit_bits, void* temp, size_t temp_bytes,
                    uint32_t* hs, int32_t* pos_s, int32_t* segid, uint64_t* uniq,
                    int32_t* seg_start, int32_t* ent_uid, int64_t p_cap, int32_t* n_uniq,
                    float* zero_a, hipStream_t st) {
  if (n_max <= 0) return;
  if (bits > 32) throw std::runtime_error("sort_rle32_dev needs key bits <= 32");
  if (temp_bytes < sort32_dev_temp_bytes(n_max))
    throw std::runtime_error("sort_rle32_dev temp too small");
  const int64_t T = (n_max + kTile - 1) / kTile;
  char* p = (char*)temp;
  uint32_t* kt = (uint32_t*)p;
  p += (size_t)n_max * 4;
  int32_t* vt = (int32_t*)p;
  p += (size_t)n_max * 4;
  uint32_t* hist = (uint32_t*)p;
  p += (size_t)kMaxDigits * T * 4;
  uint32_t* part = (uint32_t*)p;
  p += (size_t)T * 4;
  uint32_t* spart = (uint32_t*)p;
  if (digit_bits == 10)
    radix32_dev<10>(keys_in, tile_cnt, n_max, T, n_dev, bits, kt, vt, hist, spart, hs, pos_s, st);
  else
    radix32_dev<8>(keys_in, tile_cnt, n_max, T, n_dev, bits, kt, vt, hist, spart, hs, pos_s, st);
  rle32_count_kernel<<<(unsigned)T, kBlk, 0, st>>>(hs, n_max, part, n_dev);
  PSAMD_HIP_CHECK(hipGetLastError());
  scan2_u32(part, T, spart, st, n_dev, n_max, 1);
  rle32_write_kernel<<<(unsigned)T, kBlk, 0, st>>>(hs, pos_s, n_max, part, segid, uniq, seg_start,
                                                   ent_uid, n_uniq, zero_a, nullptr, n_dev, p_cap);
  PSAMD_HIP_CHECK(hipGetLastError());
}

}  // namespace psamd
