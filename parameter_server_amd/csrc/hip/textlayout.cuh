// The layout half of the text writers (modeltext.hip, scoretext.hip): variable-length
// records formatted by fixed blocks of entries, one workgroup a block, in three launches
// (count -> scan -> emit). What the writers share is here: the header words, the scan of
// one word per thread over a workgroup, the kernel that turns the blocks' byte totals into
// offsets and checks the sum against the capacity, and the copy of a block's text from LDS
// to its byte range with 16-byte stores. Each writer adds its own count and emit kernels
// (they know the record). Included by .hip files only; everything has internal linkage.
#pragma once
#include "common.cuh"

#include <cstdint>

namespace psamd {

namespace {

constexpr int kMtScanBlk = 1024;

// header words (int64)
enum { H_BYTES, H_DEFER, H_OVER, H_WORDS };

// Exclusive scan of one word per thread over a workgroup of kWaves waves. lds: kWaves + 1.
template <int kWaves>
__device__ __forceinline__ uint32_t mt_block_scan(uint32_t v, uint32_t* lds, uint32_t* total) {
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
    for (int w = 0; w < kWaves; ++w) {
      const uint32_t t = lds[w];
      lds[w] = run;
      run += t;
    }
    lds[kWaves] = run;
  }
  __syncthreads();
  const uint32_t res = lds[wid] + x - v;
  *total = lds[kWaves];
  __syncthreads();
  return res;
}

__global__ void __launch_bounds__(kMtScanBlk) mt_scan_kernel(const uint32_t* __restrict__ totals,
                                                             int64_t nb, int64_t cap,
                                                             int64_t* __restrict__ offs,
                                                             unsigned long long* __restrict__ hdr) {
  __shared__ uint32_t lds[kMtScanBlk / kWave + 1];
  int64_t run = 0;  // (the same in every thread; a tile is < 2^26 bytes)
  for (int64_t c = 0; c < nb; c += kMtScanBlk) {
    const int64_t b = c + threadIdx.x;
    const uint32_t t = b < nb ? totals[b] : 0u;
    uint32_t tile;
    const uint32_t ex = mt_block_scan<kMtScanBlk / kWave>(t, lds, &tile);
    if (b < nb) offs[b] = run + ex;
    run += tile;
  }
  if (threadIdx.x == 0) {
    hdr[H_BYTES] = (unsigned long long)run;
    hdr[H_OVER] = run > cap ? 1ull : 0ull;
  }
}

// The block's text, LDS bytes [shift, shift + total) with shift = (out + goff) mod 16, to
// out[goff, goff + total): lds byte q <-> out[goff - shift + q], so 16-byte pieces are
// aligned on both sides. Whole pieces go out as one 16-byte store, consecutive lanes to
// consecutive addresses; the first and last partial piece as single bytes. Call after the
// barrier that completes the text. kBlk: threads per workgroup.
template <int kBlk>
__device__ __forceinline__ void mt_copy_out(const uint8_t* text, uint32_t shift, uint32_t total,
                                            uint8_t* out, int64_t goff) {
  uint8_t* base = out + goff - shift;
  const uint32_t lo = shift, hi = shift + total;
  const uint32_t npieces = (hi + 15u) >> 4;
  for (uint32_t pc = threadIdx.x; pc < npieces; pc += kBlk) {
    const uint32_t q = pc << 4;
    if (q >= lo && q + 16u <= hi) {
      *reinterpret_cast<uint4*>(base + q) = *reinterpret_cast<const uint4*>(text + q);
    } else {
      for (uint32_t b = q < lo ? lo : q; b < q + 16u && b < hi; ++b) base[b] = text[b];
    }
  }
}

// work buffer of a writer over nb blocks: int64 offsets, then uint32 totals
inline int64_t mt_work_bytes(int64_t nb) { return nb * 8 + ((nb * 4 + 15) / 16) * 16 + 16; }

}  // namespace

}  // namespace psamd
