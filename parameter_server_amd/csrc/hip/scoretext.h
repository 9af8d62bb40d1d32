// Host entry points of scoretext.hip: prediction lines (one or two f32 columns a row)
// formatted on the GPU.
#pragma once
#include <hip/hip_runtime.h>
#include <cstdint>

namespace psamd {

int64_t scoretext_block();              // rows per workgroup
int64_t scoretext_max_line(int ncols);  // bytes one line of ncols (1 or 2) columns can take
int64_t scoretext_work_bytes(int64_t n);
// Row i becomes "first[i]\n" (second == nullptr) or "first[i]\tsecond[i]\n", each column as
// Python's "%.9g" % float(x). first / second: n f32 bit patterns each; n may be 0;
// cap: capacity of out in bytes; hdr: 3 result words {text bytes, values the formatter
// deferred, total over cap}; work: >= scoretext_work_bytes(n) bytes, 8-byte aligned.
// With a deferred value or an overflow the text is not to be used (with an overflow nothing
// was written).
void scoretext_format(const uint32_t* first, const uint32_t* second, int64_t n, uint8_t* out,
                      int64_t cap, int64_t* hdr, uint8_t* work, hipStream_t st);

}  // namespace psamd
