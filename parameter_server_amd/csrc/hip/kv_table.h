// Host entry points of kv_table.hip: the open-addressing slot table (32-B slots).
// slots / cap: the table and its capacity (a power of two). Counts named *_cap are
// capacities of the buffer before them; n_dev (may be null) is a device count that
// clamps n.
#pragma once
#include <hip/hip_runtime.h>
#include <cstdint>

#include "kv_slot.cuh"
#include "params.h"

namespace psamd {

// every key slot to kEmptyKey, the values to zero
void kv_init(void* slots, int64_t cap, hipStream_t st);
// every occupied slot of the old table into `t` (kv_init-ed, not smaller); moved: striped
// u64 count of slots moved; err (may be null): bit 0 = new table exhausted
void kv_rehash(const void* old_slots, int64_t old_cap, const TableRef& t,
               unsigned long long* moved, int stripes, int32_t* err, hipStream_t st);
// warm start: n (raw key, weight) pairs into the table with the optimizer state of rule p
// that reproduces each weight (n0: prior gradient norm); keeps mixed keys in [lo, last];
// counts: count_stripes x kAccStride u64 [seeded, overwritten, foreign, out_of_range,
// skipped], added to; stats.ptr (may be null): [0] += change of the non-zero weight
// count; err (may be null): bit 0 = table full. Runs alone on the table
void kv_seed(const TableRef& t, KeyMix km, const uint64_t* raw, const float* w, int64_t n,
             uint64_t lo, uint64_t last, const UpdateParams& p, float n0,
             unsigned long long* counts, int count_stripes, const StripedAcc& stats,
             int32_t* err, hipStream_t st);
// slot index (-1: absent / full) and weight of n keys; out_w, err, inserted may be null
void kv_resolve(const TableRef& t, const uint64_t* keys, int64_t n, const int32_t* n_dev,
                int64_t* out_slot, float* out_w, bool insert, const KeyInit& init, int32_t* err,
                int32_t* inserted, hipStream_t st);
// the same for the keys of G received exchange rows (H words, <= C keys of kw words);
// out_w row stride wstride (0 = C); out_key, bnd (partition bounds, ordered home only)
// may be null
void kv_resolve_rows(const TableRef& t, const int32_t* recv, int G, int64_t H, int64_t C, int kw,
                     int64_t* out_slot, float* out_w, int64_t wstride, bool insert,
                     const KeyInit& init, int32_t* err, int32_t* inserted, uint64_t* out_key,
                     int32_t* bnd, int lgP, hipStream_t st);
// out[i] = field (0..3: w, z, n, acc) of slot slot_idx[i]
void kv_gather(const void* slots, int64_t cap, const int64_t* slot_idx, int64_t n,
               const int32_t* n_dev, float* out, int field, hipStream_t st);
// w / z / nn (each may be null) into the slots
void kv_set(void* slots, int64_t cap, const int64_t* slot_idx, int64_t n, const float* w,
            const float* z, const float* nn, hipStream_t st);
// one optimizer step per (slot, gradient); stats.ptr may be null; auc.hist null = no AUC
void kv_update(void* slots, int64_t cap, const int64_t* slot_idx, const float* grad, int64_t n,
               const int32_t* n_dev, const UpdateParams& p, const StripedAcc& stats,
               const AucOut& auc, hipStream_t st);
// aggregated push: gradients summed into the slots' acc, first touchers listed
void kv_accumulate(void* slots, int64_t cap, const int64_t* slot_idx, const float* grad,
                   int64_t n, const int32_t* n_dev, int64_t* touched, int32_t* n_touched,
                   int64_t touched_cap, hipStream_t st);
// the same over G source rows; gradient row s at grad[s * gstride]
void kv_accumulate_rows(void* slots, int64_t cap, const int64_t* slot_idx, const float* grad,
                        int64_t gstride, const int32_t* recv, int G, int64_t H, int64_t C,
                        int64_t* touched, int32_t* n_touched, int64_t touched_cap,
                        hipStream_t st);
// one optimizer step per touched slot from its acc; max_n: capacity of touched
void kv_apply_accumulated(void* slots, int64_t cap, const int64_t* touched,
                          const int32_t* n_touched, int64_t max_n, const UpdateParams& p,
                          const StripedAcc& stats, hipStream_t st);
// per-push apply of G source rows in row order per slot; link: scratch of link_size
// (a power of two >= 2*G*C) words, nxt: G*C words
void kv_update_rows(void* slots, int64_t cap, const int64_t* slot_idx, const float* grad,
                    int64_t gstride, const int32_t* recv, int G, int64_t H, int64_t C,
                    unsigned long long* link, int64_t link_size, int32_t* nxt,
                    const UpdateParams& p, const StripedAcc& stats, hipStream_t st);
// the same partitioned by key range (bnd: G x (2^lgP + 1) bounds); ffnb > 0: the
// gradients are the rows' FixingFloat codes of ffnb bytes (grad unused)
void kv_apply_part(void* slots, int64_t cap, const int64_t* slot_idx, const uint64_t* keys,
                   const float* grad, int64_t gstride, const int32_t* recv, int G, int64_t H,
                   int64_t C, const int32_t* bnd, int lgP, const UpdateParams& p,
                   const StripedAcc& stats, int ffnb, int kw, hipStream_t st);
// out: the table's two u64 census counters (kv_census_kernel), added to, not zeroed
void kv_census(const void* slots, int64_t cap, unsigned long long* out, hipStream_t st);

}  // namespace psamd
