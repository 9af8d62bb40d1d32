// Host entry points of tploc.hip / tploc_bucket.hip / tploc_flat.hip / tploc_fused.hip /
// tploc_step.hip: tile dedup + bucket partition localisation ("tp"), its flat 1-GPU layout
// ("tpf"), the fused forward / backward and the fused step (device helpers: tploc.cuh,
// host: tploc_geom.h).
// n: keys of the minibatch; bits: key bits (KeyMix); *_cap: capacity of the buffer
// before it. Entry buffers hold >= tploc_stride(n) (tp) / tpf_stride(n) (tpf) elements.
#pragma once
#include <hip/hip_runtime.h>
#include <cstddef>
#include <cstdint>

#include "countmin.cuh"
#include "kv_slot.cuh"
#include "params.h"

namespace psamd {

// ---- geometry (host only)
int64_t tploc_stride(int64_t n);    // entry stride of n keys
int64_t tpf_stride(int64_t n);      // the same, flat layout
int64_t tpf_stride_max(int64_t n);  // bound of tpf_stride over minibatches of <= n keys
int tpf_tile_log2(int64_t n);
int tploc_buckets(int64_t n, int bits);
int tploc_tile();
bool tploc_supported(int64_t n, int bits);  // 2..34 key bits, n <= 5.2 M
size_t tploc_temp_bytes(int64_t n, int bits);
int tpf_groups(int64_t n, int bits);  // bucket groups = workgroups of the flat kernels
int tpf_key_region();                 // keys / entries a group's region holds
int tpf_entry_region();
int tpf_xcd_group(int bid, int groups);       // logical group of physical block bid
size_t tpf_temp_bytes(int64_t n, int bits);   // (any minibatch of <= n keys)
bool tpf_exchange_ok(int64_t n, int bits, int G);  // G a power of two dividing the groups
bool tp_fwd_bwd_supported(int width);              // fixed row width 9..64

// phase marks of the tile / fused kernel (tuning aid): 16 u64 per tile, null = off
void tp_tile_set_prof(uint64_t* p);
void tp_fb_set_prof(uint64_t* p);

// ---- tp layout
// local_col, pieces, prof may be null; u_cap: capacity of uniq
void localize_tp(const uint64_t* raw, int64_t n, KeyMix m, void* temp, size_t temp_bytes,
                 int32_t* dcnt, uint16_t* rep, int32_t* pos_s, int32_t* segid, uint64_t* uniq,
                 int32_t* seg_start, int32_t* ent_uid, int32_t* local_col, int32_t* n_uniq,
                 int32_t* n_ent, float* grad, unsigned long long* pieces, int32_t* err,
                 int64_t u_cap, uint64_t* prof, hipStream_t st);
// rows null: fixed row width; vals null: binary features; B: capacity of coef
void tp_backward(const uint16_t* rep, const int32_t* dcnt, int64_t n, const int32_t* rows,
                 int width, const float* vals, const float* coef, int64_t B, float* psum,
                 const int32_t* pos_s, const int32_t* segid, const int32_t* n_ent, float* grad,
                 int64_t grad_cap, hipStream_t st);
void tp_gather(const uint16_t* rep, const int32_t* ent_uid, int64_t n, int32_t* local_col,
               hipStream_t st);
// ent_uid null: the flat layout (w_local in tile-entry order; pos_s / segid / n_ent /
// grad unused, reduce false). vals, metrics, hist may be null.
void tp_fwd_bwd(const uint16_t* rep, const int32_t* dcnt, const int32_t* ent_uid, int64_t n,
                int width, const float* vals, const float* w_local, int64_t w_cap,
                const float* labels, int64_t B, int loss_type, float* coef_out, double* metrics,
                uint32_t* hist, int nbins, int acc_stripes, int hist_stripes, float* psum,
                const int32_t* pos_s, const int32_t* segid, const int32_t* n_ent, float* grad,
                int64_t grad_cap, bool reduce, hipStream_t st);
// variable-width / valued rows: row_ptr [B + 1], rows [n] (row of every occurrence)
void tp_fwd_bwd_csr(const uint16_t* rep, const int32_t* dcnt, const int32_t* ent_uid, int64_t n,
                    const int64_t* row_ptr, const int32_t* rows, const float* vals,
                    const float* w_local, int64_t w_cap, const float* labels, int64_t B,
                    int loss_type, float* coef_out, double* metrics, uint32_t* hist, int nbins,
                    int acc_stripes, int hist_stripes, float* psum, const int32_t* pos_s,
                    const int32_t* segid, const int32_t* n_ent, float* grad, int64_t grad_cap,
                    bool reduce, hipStream_t st);
// fused segment scan + optimizer step; acc: the localiser's pieces, u_cap its capacity
void tp_seg_update(const int32_t* pos_s, const int32_t* segid, int64_t n, const int32_t* n_ent,
                   const float* psum, const int32_t* seg_start, const int32_t* n_uniq,
                   unsigned long long* acc, int64_t u_cap, const int64_t* slot_idx, void* slots,
                   int64_t cap, const UpdateParams& p, const StripedAcc& stats,
                   const AucOut& auc, hipStream_t st);

// ---- flat layout
// filt null: no tail filter (then ecnt / w_ent unused); cnt_pre may be null;
// stage 0 = all, 1 tile, 2 bucket, 3 tail filter, 4 tile + bucket
void localize_tpf(const uint64_t* raw, int64_t n, KeyMix m, void* temp, size_t temp_bytes,
                  int32_t* dcnt, uint16_t* rep, uint64_t* uniqf, int32_t* ent_pos, uint16_t* ent_j,
                  int32_t* cnt, int32_t* err, bool sorted, hipStream_t st, const CmArgs* filt,
                  uint8_t* ecnt, float* w_ent, int64_t w_cap, int32_t* cnt_pre, int stage);
// the padded exchange on the flat layout: rows of H words, <= C keys of kw words per
// owner; ovf (may be null) counts keys that did not fit
void tpf_pack_keys(int64_t n, int bits, int G, const int32_t* cnt, const uint64_t* uniqf, int64_t C,
                   int kw, int64_t H, int32_t* send, int32_t* ovf, hipStream_t st);
// wstride: row stride of wrecv (0 = C)
void tpf_unpack_w(int64_t n, int bits, int G, const int32_t* cnt, const int32_t* ent_pos,
                  const uint16_t* ent_j, int64_t C, const float* wrecv, int64_t wstride,
                  float* w_ent, int64_t w_cap, hipStream_t st);
// ff: the gradients go to the f32 staging buffer gstage (FixingFloat path), not into
// the rows; auc.nbins is not read (2048); ovf / ovf_host (device-mapped host word) may
// be null
void tpf_pack_grads(int64_t n, int bits, int G, const int32_t* cnt, const int32_t* ent_pos,
                    const uint16_t* ent_j, int64_t C, int kw, int64_t H, const float* psum,
                    int64_t p_cap, int32_t* send, bool ff, float* gstage, const AucOut& auc,
                    const int32_t* ovf, int32_t* ovf_host, hipStream_t st);
// One launch over the groups of an n-key minibatch: update A then pull B (the same n).
// cntA null: pull only; cntB null: update only. err, inserted, stats.ptr may be null.
void tpf_step(int64_t n, int bits, const int32_t* cntA, const int32_t* posA, const uint16_t* jA,
              const uint32_t* slotA, const float* psum, int64_t p_cap, const int32_t* cntB,
              const uint64_t* uniqB, const int32_t* posB, const uint16_t* jB, uint32_t* slotB,
              float* w_ent, int64_t w_cap, const TableRef& t, const KeyInit& init, int32_t* err,
              int32_t* inserted, const UpdateParams& p, const StripedAcc& stats,
              const AucOut& auc, hipStream_t st);

}  // namespace psamd
