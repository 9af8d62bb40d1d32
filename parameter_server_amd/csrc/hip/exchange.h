// Host entry points of exchange.hip: the fixed-capacity (padded, sync-free) exchange.
// send / recv: G rows of H int32 words, <= C keys of kw words each (row layout in
// exchange.hip). off: [G + 1] owner offsets into the unique keys; n_host: capacity of the
// unique-key arrays (n_uniq is the device count); perm may be null.
#pragma once
#include <hip/hip_runtime.h>
#include <cstdint>

#include "params.h"

namespace psamd {

// dst: device-visible pointer of a pinned host word
void xchg_publish(const int32_t* src, int32_t* host_mapped_dst, hipStream_t st);
// ovf (may be null) counts keys that did not fit
void xchg_pack_keys(const uint64_t* ukeys, const int32_t* n_uniq, int64_t n_host,
                    const int64_t* off, int G, int64_t C, int kw, int64_t H, int32_t* send,
                    int32_t* ovf, hipStream_t st);
// auc.nbins is not read (2048); ovf / ovf_host (device-mapped host word) may be null
void xchg_pack_grads(const float* grad, const int32_t* perm, const int32_t* n_uniq,
                     int64_t n_host, const int64_t* off, int G, int64_t C, int kw, int64_t H,
                     int32_t* send, const AucOut& auc, const int32_t* ovf, int32_t* ovf_host,
                     hipStream_t st);
void xchg_clear_counts(int32_t* send, int G, int64_t H, bool keys, bool grads, hipStream_t st);
// wstride: row stride of recv_w (0 = C)
void xchg_unpack_w(const float* recv_w, const int32_t* perm, const int32_t* n_uniq,
                   int64_t n_host, const int64_t* off, int G, int64_t C, int64_t wstride,
                   float* w_local, hipStream_t st);
// FixingFloat rows: nb-byte codes (1..7); step (may be null): device step clock of the
// rounding RNG; gstage: >= G * C floats of staging
void xchg_ff_pack_grads(const float* grad, const int32_t* perm, const int32_t* n_uniq,
                        int64_t n_host, const int64_t* off, int G, int64_t C, int kw, int64_t H,
                        int nb, uint64_t seed, const int64_t* step, int32_t* send, float* gstage,
                        hipStream_t st);
// per > 0: gstage carries 2 * G * per min / max partials behind the G * C gradients
void xchg_ff_encode(const float* gstage, int G, int64_t C, int kw, int64_t H, int nb, uint64_t seed,
                    const int64_t* step, int32_t* send, int per, hipStream_t st);
void xchg_ff_decode(const int32_t* recv, int G, int64_t C, int kw, int64_t H, int nb, float* gin,
                    hipStream_t st);

}  // namespace psamd
