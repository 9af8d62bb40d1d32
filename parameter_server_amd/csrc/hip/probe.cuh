// Read-only probes of the slot table, shared by the scoring kernels (predict.hip,
// fm_predict.hip): the 16-byte slot head and the walk along a chain after a first-probe
// miss. Nothing here stores to the table.
#pragma once
#include "kv_slot.cuh"

namespace psamd {

// {key, w, z} of a slot as one 16-byte load (Slot is 32-byte aligned)
__device__ __forceinline__ uint4 load_slot_head(const Slot* __restrict__ slots, uint64_t idx) {
  return *reinterpret_cast<const uint4*>(slots + idx);
}
__device__ __forceinline__ uint64_t head_key(const uint4& v) {
  return ((uint64_t)v.y << 32) | v.x;
}

// The rest of a probe chain whose first slot (idx) held another key. Read-only. Returns
// the slot that holds h (-1: absent) and its weight through w (0 if absent).
__device__ __forceinline__ int64_t probe_on(const Slot* __restrict__ slots, uint64_t mask,
                                            uint64_t idx, uint64_t h, float& w) {
  w = 0.f;
  // TRIP BOUND: at most mask + 1 slots are visited in all (the first probe was slot 0 of
  // the chain), as in resolve_key: on a table without an empty slot an absent key's
  // chain never meets kEmptyKey, and without the bound this loop would not end.
  for (uint64_t probe = 1; probe <= mask; ++probe) {
    idx = (idx + 1) & mask;
    const uint4 v = load_slot_head(slots, idx);
    const uint64_t k = head_key(v);
    if (k == h) {
      w = __uint_as_float(v.z);
      return (int64_t)idx;
    }
    if (k == kEmptyKey) return -1;
  }
  return -1;
}

}  // namespace psamd
