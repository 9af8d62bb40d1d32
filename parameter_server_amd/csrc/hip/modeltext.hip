// (raw key u64, weight f32) arrays -> key<TAB>weight text on the device (gfx950): the
// device half of utils/checkpoint.write_text_model, byte for byte. The conversion itself is
// ../core/textfmt.h (integer arithmetic only, shared with the host); this file lays the
// entries out (the scan and the copy-out are textlayout.cuh, shared with scoretext.hip). A
// strict fast path: an entry outside the formatter's exact domain raises the header's
// deferred count and the caller formats the whole chunk on the host.
//
// One workgroup owns a fixed block of kMtEntries = 1024 consecutive entries (256 threads x
// 4 entries). Three launches, no hand-off between workgroups inside a launch:
//   1. mt_count  every entry's text length -> one byte total per block, deferred entries
//                -> header.
//   2. mt_scan   one workgroup scans the block totals: each block's byte offset, the
//                chunk's total (checked against the output capacity).
//   3. mt_emit   converts its block again (the conversion is cheaper than a round trip of
//                the digits through memory), scans the lengths in the workgroup, assembles
//                the block's text in LDS -- at most 37 bytes an entry, placed so that LDS
//                and global addresses agree mod 16 -- and copies it out with 16-byte
//                stores, consecutive lanes to consecutive addresses; only the block's
//                first and last partial 16 bytes go out as single bytes.
// Traffic: keys and weights are read twice (12 B an entry each time), the text is written
// once.
//
// Safety: every entry index is checked against n, the chunk total against the capacity
// before anything is emitted (H_OVER; mt_emit then writes nothing), and a block writes
// only [offset, offset + its own total), which the scan made disjoint and in range.
//
// Resources (hipcc -O3 --offload-arch=gfx950 -Rpass-analysis=kernel-resource-usage):
//   mt_count_kernel  VGPRs 30, SGPRs 44, ScratchSize 0, LDS    32 B, occupancy 8 waves/SIMD
//   mt_scan_kernel   VGPRs 40, SGPRs 36, ScratchSize 0, LDS    68 B, occupancy 8
//   mt_emit_kernel   VGPRs 55, SGPRs 52, ScratchSize 0, LDS 37924 B, occupancy 4 (LDS: four
//                    workgroups of four waves a CU)
#include "modeltext.h"
#include "common.cuh"
#include "textlayout.cuh"
#include "../core/textfmt.h"

#include <stdexcept>

namespace psamd {

namespace {

constexpr int kMtBlk = 256;                     // threads per workgroup
constexpr int kMtPer = 4;                       // entries per thread
constexpr int kMtEntries = kMtBlk * kMtPer;     // entries per workgroup
constexpr int kMtWaves = kMtBlk / kWave;
constexpr int kMtLds = kMtEntries * textfmt::kMaxEntry + 16;  // + the mod-16 shift

// The text length of entry i (0 when the formatter does not decide it).
__device__ __forceinline__ int mt_entry(const uint64_t* __restrict__ keys,
                                        const uint32_t* __restrict__ wbits, int64_t i,
                                        uint64_t* key, textfmt::Dec* d, int* klen, int* st) {
  *key = keys[i];
  *st = textfmt::dec_f32(wbits[i], d);
  if (*st != textfmt::kOk) return 0;
  *klen = textfmt::key_len(*key);
  return *klen + textfmt::weight_len(*d) + 2;
}

__global__ void __launch_bounds__(kMtBlk) mt_count_kernel(const uint64_t* __restrict__ keys,
                                                          const uint32_t* __restrict__ wbits,
                                                          int64_t n, uint32_t* __restrict__ totals,
                                                          unsigned long long* __restrict__ hdr) {
  __shared__ uint32_t red[2][kMtWaves];
  const int64_t i0 = (int64_t)blockIdx.x * kMtEntries + (int64_t)threadIdx.x * kMtPer;
  uint32_t bytes = 0, defer = 0;
#pragma unroll
  for (int j = 0; j < kMtPer; ++j) {
    if (i0 + j >= n) break;
    uint64_t key;
    textfmt::Dec d;
    int kl, st;
    bytes += (uint32_t)mt_entry(keys, wbits, i0 + j, &key, &d, &kl, &st);
    defer += st != textfmt::kOk;
  }
  bytes = wave_sum(bytes);
  defer = wave_sum(defer);
  const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
  if (lane == 0) {
    red[0][wid] = bytes;
    red[1][wid] = defer;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    uint32_t b = 0, f = 0;
    for (int w = 0; w < kMtWaves; ++w) {
      b += red[0][w];
      f += red[1][w];
    }
    totals[blockIdx.x] = b;
    if (f) atomicAdd(&hdr[H_DEFER], (unsigned long long)f);
  }
}

__global__ void __launch_bounds__(kMtBlk) mt_emit_kernel(const uint64_t* __restrict__ keys,
                                                         const uint32_t* __restrict__ wbits,
                                                         int64_t n, const int64_t* __restrict__ offs,
                                                         uint8_t* __restrict__ out, int64_t cap,
                                                         const unsigned long long* __restrict__ hdr) {
  __shared__ __attribute__((aligned(16))) uint8_t text[kMtLds];
  __shared__ uint32_t lds_scan[kMtWaves + 1];
  if (hdr[H_OVER]) return;  // (uniform: set before this launch)
  const int64_t goff = offs[blockIdx.x];
  const uint32_t shift = (uint32_t)((uintptr_t)(out + goff) & 15u);
  const int64_t i0 = (int64_t)blockIdx.x * kMtEntries + (int64_t)threadIdx.x * kMtPer;

  uint64_t key[kMtPer];
  textfmt::Dec d[kMtPer];
  int kl[kMtPer], len[kMtPer];
  uint32_t mine = 0;
#pragma unroll
  for (int j = 0; j < kMtPer; ++j) {
    len[j] = 0;
    kl[j] = 0;
    if (i0 + j < n) {
      int st;
      len[j] = mt_entry(keys, wbits, i0 + j, &key[j], &d[j], &kl[j], &st);
    }
    mine += (uint32_t)len[j];
  }
  uint32_t total;
  uint32_t o = shift + mt_block_scan<kMtWaves>(mine, lds_scan, &total);
#pragma unroll
  for (int j = 0; j < kMtPer; ++j) {
    if (len[j] == 0) continue;
    // (o + len <= shift + total <= 15 + kMtEntries * kMaxEntry < kMtLds)
    uint8_t* p = text + o;
    textfmt::put_key(key[j], kl[j], p);
    p[kl[j]] = '\t';
    const int wl = textfmt::put_weight(d[j], p + kl[j] + 1);
    p[kl[j] + 1 + wl] = '\n';
    o += (uint32_t)len[j];
  }
  __syncthreads();
  if (goff < 0 || goff + (int64_t)total > cap) return;  // (never: the scan checked the sum)
  mt_copy_out<kMtBlk>(text, shift, total, out, goff);
}

}  // namespace

int64_t modeltext_block() { return kMtEntries; }
int64_t modeltext_max_entry() { return textfmt::kMaxEntry; }
int64_t modeltext_work_bytes(int64_t n) {
  return mt_work_bytes((n + kMtEntries - 1) / kMtEntries);
}

// Formats n sorted entries into out (cap bytes). hdr: 3 int64 {text bytes, entries the
// formatter deferred, total over capacity}; work: modeltext_work_bytes(n), 8-byte aligned.
// With a deferred entry or an overflow the text is not to be used.
void modeltext_format(const uint64_t* keys, const uint32_t* wbits, int64_t n, uint8_t* out,
                      int64_t cap, int64_t* hdr, uint8_t* work, hipStream_t st) {
  if (n <= 0 || n > ((int64_t)1 << 28))
    throw std::invalid_argument("modeltext_format: entries per call must be in [1, 2^28]");
  if (((uintptr_t)work & 7) != 0 || ((uintptr_t)hdr & 7) != 0)
    throw std::invalid_argument("modeltext_format: work and hdr must be 8-byte aligned");
  const int64_t nb = (n + kMtEntries - 1) / kMtEntries;
  int64_t* offs = reinterpret_cast<int64_t*>(work);
  uint32_t* totals = reinterpret_cast<uint32_t*>(work + nb * 8);
  auto* h = reinterpret_cast<unsigned long long*>(hdr);
  PSAMD_HIP_CHECK(hipMemsetAsync(hdr, 0, H_WORDS * sizeof(int64_t), st));
  mt_count_kernel<<<(unsigned)nb, kMtBlk, 0, st>>>(keys, wbits, n, totals, h);
  mt_scan_kernel<<<1, kMtScanBlk, 0, st>>>(totals, nb, cap, offs, h);
  mt_emit_kernel<<<(unsigned)nb, kMtBlk, 0, st>>>(keys, wbits, n, offs, out, cap, h);
  PSAMD_HIP_CHECK(hipGetLastError());
}

}  // namespace psamd
