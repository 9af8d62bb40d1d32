// f32 columns -> prediction lines on the device (gfx950): row i of one column is
// "%.9g\n" % first[i], of two columns "%.9g\t%.9g\n" % (first[i], second[i]) -- what the host
// loop of ops/scoretext.py writes, byte for byte. The kernels only format floats (a
// probability is a torch op applied before them). The conversion is textfmt::dec_score of
// ../core/textfmt.h (integer arithmetic only, shared with the host; +-0 are in its domain:
// a margin of +0 is every row without a key in the model); the layout is the one of
// modeltext.hip, its shared parts in textlayout.cuh. A strict fast path: a value outside
// the formatter's exact domain (inf, nan, subnormals, |x| >= 1e9, 0 < |x| < 1e-22) raises
// the header's deferred count and the caller formats the whole chunk on the host.
//
// One workgroup owns a fixed block of kStEntries = 1024 consecutive rows (256 threads x 4
// rows). Three launches, no hand-off between workgroups inside a launch:
//   1. st_count  every row's text length -> one byte total per block, deferred values ->
//                header.
//   2. mt_scan   (textlayout.cuh) the blocks' byte offsets and the chunk's total, checked
//                against the output capacity.
//   3. st_emit   converts its block again, scans the lengths in the workgroup, assembles
//                the block's text in LDS -- at most 16 bytes a column, placed so that LDS
//                and global addresses agree mod 16 -- and copies it out with 16-byte
//                stores (mt_copy_out).
// Traffic: each column is read twice (4 B a value each time), the text is written once.
//
// Safety: every row index is checked against n, the chunk total against the capacity
// before anything is emitted (H_OVER; st_emit then writes nothing), and a block writes
// only [offset, offset + its own total), which the scan made disjoint and in range. A row
// with a deferred value has length 0 in both passes.
//
// Resources (hipcc -O3 --offload-arch=gfx950 -Rpass-analysis=kernel-resource-usage):
//   st_count_kernel<1>  VGPRs 32, SGPRs 46, ScratchSize 0, LDS    32 B, occupancy 8 waves/SIMD
//   st_count_kernel<2>  VGPRs 31, SGPRs 52, ScratchSize 0, LDS    32 B, occupancy 8
//   st_emit_kernel<1>   VGPRs 39, SGPRs 46, ScratchSize 0, LDS 16420 B, occupancy 8
//   st_emit_kernel<2>   VGPRs 51, SGPRs 56, ScratchSize 0, LDS 32804 B, occupancy 4 (LDS: four
//                       workgroups of four waves a CU)
//   mt_scan_kernel      VGPRs 40, SGPRs 36, ScratchSize 0, LDS    68 B, occupancy 8
#include "scoretext.h"
#include "common.cuh"
#include "textlayout.cuh"
#include "../core/textfmt.h"

#include <stdexcept>

namespace psamd {

namespace {

constexpr int kStBlk = 256;                  // threads per workgroup
constexpr int kStPer = 4;                    // rows per thread
constexpr int kStEntries = kStBlk * kStPer;  // rows per workgroup
constexpr int kStWaves = kStBlk / kWave;
constexpr int kStCol = textfmt::kMaxScore + 1;  // a column and its separator

// The text length of row i (0 when the formatter does not decide one of its values);
// *defer: how many of its values it did not decide.
template <int kCols>
__device__ __forceinline__ int st_row(const uint32_t* __restrict__ first,
                                      const uint32_t* __restrict__ second, int64_t i,
                                      textfmt::Dec* d, int* defer) {
  int len = 0;
  *defer = 0;
#pragma unroll
  for (int c = 0; c < kCols; ++c) {
    const uint32_t bits = c == 0 ? first[i] : second[i];
    if (textfmt::dec_score(bits, &d[c]) != textfmt::kOk)
      ++*defer;
    else
      len += textfmt::weight_len(d[c]) + 1;
  }
  return *defer ? 0 : len;
}

template <int kCols>
__global__ void __launch_bounds__(kStBlk) st_count_kernel(const uint32_t* __restrict__ first,
                                                          const uint32_t* __restrict__ second,
                                                          int64_t n, uint32_t* __restrict__ totals,
                                                          unsigned long long* __restrict__ hdr) {
  __shared__ uint32_t red[2][kStWaves];
  const int64_t i0 = (int64_t)blockIdx.x * kStEntries + (int64_t)threadIdx.x * kStPer;
  uint32_t bytes = 0, defer = 0;
#pragma unroll
  for (int j = 0; j < kStPer; ++j) {
    if (i0 + j >= n) break;
    textfmt::Dec d[kCols];
    int df;
    bytes += (uint32_t)st_row<kCols>(first, second, i0 + j, d, &df);
    defer += (uint32_t)df;
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
    for (int w = 0; w < kStWaves; ++w) {
      b += red[0][w];
      f += red[1][w];
    }
    totals[blockIdx.x] = b;
    if (f) atomicAdd(&hdr[H_DEFER], (unsigned long long)f);
  }
}

template <int kCols>
__global__ void __launch_bounds__(kStBlk) st_emit_kernel(const uint32_t* __restrict__ first,
                                                         const uint32_t* __restrict__ second,
                                                         int64_t n, const int64_t* __restrict__ offs,
                                                         uint8_t* __restrict__ out, int64_t cap,
                                                         const unsigned long long* __restrict__ hdr) {
  constexpr int kLds = kStEntries * kCols * kStCol + 16;  // + the mod-16 shift
  __shared__ __attribute__((aligned(16))) uint8_t text[kLds];
  __shared__ uint32_t lds_scan[kStWaves + 1];
  if (hdr[H_OVER]) return;  // (uniform: set before this launch)
  const int64_t goff = offs[blockIdx.x];
  const uint32_t shift = (uint32_t)((uintptr_t)(out + goff) & 15u);
  const int64_t i0 = (int64_t)blockIdx.x * kStEntries + (int64_t)threadIdx.x * kStPer;

  textfmt::Dec d[kStPer][kCols];
  int len[kStPer];
  uint32_t mine = 0;
#pragma unroll
  for (int j = 0; j < kStPer; ++j) {
    len[j] = 0;
    if (i0 + j < n) {
      int df;
      len[j] = st_row<kCols>(first, second, i0 + j, d[j], &df);
    }
    mine += (uint32_t)len[j];
  }
  uint32_t total;
  uint32_t o = shift + mt_block_scan<kStWaves>(mine, lds_scan, &total);
#pragma unroll
  for (int j = 0; j < kStPer; ++j) {
    if (len[j] == 0) continue;
    // (o + len <= shift + total <= 15 + kStEntries * kCols * kStCol < kLds)
    uint8_t* p = text + o;
#pragma unroll
    for (int c = 0; c < kCols; ++c) {
      p += textfmt::put_weight(d[j][c], p);
      *p++ = c + 1 < kCols ? '\t' : '\n';
    }
    o += (uint32_t)len[j];
  }
  __syncthreads();
  if (goff < 0 || goff + (int64_t)total > cap) return;  // (never: the scan checked the sum)
  mt_copy_out<kStBlk>(text, shift, total, out, goff);
}

template <int kCols>
void st_launch(const uint32_t* first, const uint32_t* second, int64_t n, int64_t nb,
               uint32_t* totals, int64_t* offs, uint8_t* out, int64_t cap,
               unsigned long long* h, hipStream_t st) {
  st_count_kernel<kCols><<<(unsigned)nb, kStBlk, 0, st>>>(first, second, n, totals, h);
  mt_scan_kernel<<<1, kMtScanBlk, 0, st>>>(totals, nb, cap, offs, h);
  st_emit_kernel<kCols><<<(unsigned)nb, kStBlk, 0, st>>>(first, second, n, offs, out, cap, h);
}

}  // namespace

int64_t scoretext_block() { return kStEntries; }
int64_t scoretext_max_line(int ncols) { return (int64_t)ncols * kStCol; }
int64_t scoretext_work_bytes(int64_t n) {
  return mt_work_bytes((n + kStEntries - 1) / kStEntries);
}

void scoretext_format(const uint32_t* first, const uint32_t* second, int64_t n, uint8_t* out,
                      int64_t cap, int64_t* hdr, uint8_t* work, hipStream_t st) {
  if (n < 0 || n > ((int64_t)1 << 28))
    throw std::invalid_argument("scoretext_format: rows per call must be in [0, 2^28]");
  if (cap < 0) throw std::invalid_argument("scoretext_format: negative capacity");
  if (((uintptr_t)work & 7) != 0 || ((uintptr_t)hdr & 7) != 0)
    throw std::invalid_argument("scoretext_format: work and hdr must be 8-byte aligned");
  PSAMD_HIP_CHECK(hipMemsetAsync(hdr, 0, H_WORDS * sizeof(int64_t), st));
  if (n == 0) return;  // (no rows: no text, nothing deferred)
  if (!first || !out) throw std::invalid_argument("scoretext_format: null column or output");
  const int64_t nb = (n + kStEntries - 1) / kStEntries;
  int64_t* offs = reinterpret_cast<int64_t*>(work);
  uint32_t* totals = reinterpret_cast<uint32_t*>(work + nb * 8);
  auto* h = reinterpret_cast<unsigned long long*>(hdr);
  if (second)
    st_launch<2>(first, second, n, nb, totals, offs, out, cap, h, st);
  else
    st_launch<1>(first, second, n, nb, totals, offs, out, cap, h, st);
  PSAMD_HIP_CHECK(hipGetLastError());
}

}  // namespace psamd
