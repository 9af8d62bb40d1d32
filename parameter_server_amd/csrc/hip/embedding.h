// Host entry points of embedding.hip: embedding rows ([cap, D] bf16 next to the KV
// table), their padded exchange, the wide & deep head and Adam. n_dev (may be null) is a
// device count that clamps n.
#pragma once
#include <hip/hip_runtime.h>
#include <cstdint>

namespace psamd {

void emb_init_rows(const int64_t* slot, const uint64_t* keys, int64_t n, const int32_t* n_dev,
                   int64_t cap, void* rows, uint8_t* inited, int D, uint64_t seed, float scale,
                   hipStream_t st);
// out[i, :] = rows[slot[i], :]
void emb_gather_rows(const int64_t* slot, int64_t n, const int32_t* n_dev, int64_t cap,
                     const void* rows, int D, void* out, hipStream_t st);
// X0[i, :] = src[idx[local_col[i]], :] (idx may be null)
void emb_expand(const int32_t* local_col, int64_t nnz, const int64_t* idx, int64_t idx_cap,
                const void* src, int64_t src_rows, int D, void* X0, hipStream_t st);
// floats of `part` emb_grad_reduce needs (0: none)
int64_t emb_grad_part_floats(int64_t nnz, int D);
bool emb_grad_wide_ok(int D);  // g_wide rides along only with D = 128 / 256
// part: emb_grad_part_floats(nnz, D) floats or null; coef / gw null: no wide gradient
void emb_grad_reduce(const int32_t* pos_s, const int32_t* segid, const int32_t* seg_start,
                     const int32_t* n_uniq, int64_t u_cap, int64_t nnz, const void* dX0, int D,
                     float* dE, float* part, const float* coef, int width, float* gw,
                     hipStream_t st);
// grad (f32) or grad16 (bf16): one is non-null. slots non-null: also the wide update,
// wide_rule = {algo, lr_type}, wide_hyper = {alpha, beta, l1, l2, grad_scale, max_delta}
void emb_update(const int64_t* slot, int64_t n, const int32_t* n_dev, int64_t cap,
                const float* grad, const void* grad16, void* rows, float* acc, int D, float lr,
                float eps, void* slots, const float* gwide, const int* wide_rule,
                const float* wide_hyper, double* stats, int acc_stripes, hipStream_t st);
// column sums of x [B, N] bf16; s, g, out_pos may be null
void colred_bf16(const void* x, int64_t B, int N, const float* s, float* out, const float* g,
                 float* out_pos, hipStream_t st);
// db_h may be null
void wd_head(const void* h, int64_t B, int H, const float* w, const float* b, const float* wide_w,
             int64_t wide_cap, const int32_t* local_col, int S, const float* labels,
             float* coef, void* dh, float* dw, float* db, float* db_h, double* metrics,
             uint32_t* hist, int nbins, int acc_stripes, hipStream_t st);
// bc1 / bc2: bias corrections of a host step; step_dev (may be null): device step clock
// that replaces them; p16 (may be null): bf16 copy of p
void adam_update(float* p, float* g, float* m, float* v, int64_t n, float lr, float b1,
                 float b2, float eps, float bc1, float bc2, float gscale, void* p16,
                 const int64_t* step_dev, bool zero_grad, hipStream_t st);
// records [C x D bf16 | C f32] per peer chunk (Q = C * D / 2 + C words)
void emb_padded_serve(const int32_t* recv, int64_t H, int64_t C, int kw, int G,
                      const int64_t* slot, const float* w, int64_t cap, void* rows,
                      uint8_t* inited, int D, uint64_t seed, float scale, int32_t* out,
                      hipStream_t st);
void emb_unpack_records(const int32_t* in, int64_t C, int G, const int64_t* off,
                        const int32_t* n_uniq, int64_t u_cap, int D, void* rows_u, float* w_u,
                        hipStream_t st);
void emb_pack_grads(const float* dE, const float* g_wide, const int64_t* off,
                    const int32_t* n_uniq, int64_t u_cap, int64_t C, int G, int D, int32_t* out,
                    hipStream_t st);

}  // namespace psamd
