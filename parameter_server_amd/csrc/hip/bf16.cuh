// bf16 <-> fp32 on the device, shared by the factor kernels (fm.hip, ffm.hip).
#pragma once
#include <hip/hip_runtime.h>
#include <cstdint>

namespace psamd {

__device__ __forceinline__ float bf16_to_f32(uint16_t h) { return __uint_as_float((uint32_t)h << 16); }

__device__ __forceinline__ uint16_t f32_to_bf16(float f) {  // round to nearest even
  const uint32_t u = __float_as_uint(f);
  if ((u & 0x7fffffffu) > 0x7f800000u) return (uint16_t)((u >> 16) | 0x40);
  return (uint16_t)((u + 0x7fffu + ((u >> 16) & 1u)) >> 16);
}

}  // namespace psamd
