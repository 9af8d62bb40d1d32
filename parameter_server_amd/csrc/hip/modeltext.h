// Host entry points of modeltext.hip: key<TAB>weight model text formatted on the GPU.
#pragma once
#include <hip/hip_runtime.h>
#include <cstdint>

namespace psamd {

int64_t modeltext_block();      // entries per workgroup
int64_t modeltext_max_entry();  // bytes one entry can take
int64_t modeltext_work_bytes(int64_t n);
// wbits: the weights' f32 bit patterns; cap: capacity of out; hdr: 3 result words;
// work: >= modeltext_work_bytes(n) bytes
void modeltext_format(const uint64_t* keys, const uint32_t* wbits, int64_t n, uint8_t* out,
                      int64_t cap, int64_t* hdr, uint8_t* work, hipStream_t st);

}  // namespace psamd
