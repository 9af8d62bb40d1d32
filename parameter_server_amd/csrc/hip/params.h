// Argument groups of the host launchers: the runs of scalars / pointers that travel
// together from the bindings to a launch. Plain host-side structs; a launcher unpacks
// them into the kernel arguments. (The optimizer rule travels as UpdateParams,
// kv_slot.cuh, the one group a kernel takes whole.)
#pragma once
#include <cstdint>

namespace psamd {

// Initial weight of an inserted key (kv_slot.cuh init_value): InitType, value, scale, seed.
struct KeyInit {
  int type;
  float v, s;
  uint64_t seed;
};

// A slot table: cap 32-B slots (a power of two) and its home map. home_m = 0: hashed
// home slots; else the ordered home of the mixed-key range starting at home_base.
struct TableRef {
  void* slots;
  int64_t cap;
  uint64_t home_base, home_m;
};

// A contended f64 accumulator (common.cuh acc_stripe): `stripes` copies kAccStride
// doubles apart, summed by the reader. ptr may be null (nothing accumulated).
struct StripedAcc {
  double* ptr;
  int stripes;
};

// The step's AUC folded into a launch: hist = stripes x 2 x nbins u32 counts, reduced
// by one block into metrics (and step_counter incremented). hist null: no AUC; metrics
// is required with hist, step_counter may be null.
struct AucOut {
  uint32_t* hist;
  int nbins, stripes;
  double* metrics;
  int64_t* step_counter;
};

}  // namespace psamd
