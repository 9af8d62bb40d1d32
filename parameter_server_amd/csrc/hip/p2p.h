// Host entry points of p2p.hip: the one-sided peer-HBM exchange and its IPC helpers.
// G ranks (1..64), self = this rank; rows of H words, <= C keys of kw words.
#pragma once
#include <hip/hip_runtime.h>
#include <cstddef>
#include <cstdint>

#include "params.h"

namespace psamd {

// tabs: 5 int64 per rank (the peers' tables); inserted may be null
void p2p_lookup_rows(const void* tabs, int G, int self, const int32_t* send, int64_t H,
                     int64_t C, int kw, float* wout, int64_t* slot_out, const KeyInit& init,
                     int32_t* err, int32_t* inserted, hipStream_t st);
// rings / applied: G device pointers; nb: FixingFloat bytes (0 = f32); Q: ring entries;
// err_host (device-mapped host word) may be null; spin: wait bound
void p2p_post(const int32_t* send, int64_t H, int64_t C, int kw, int nb, int G, int self,
              int32_t seq, int Q, void* const* rings, void* const* applied, int32_t* ok,
              int32_t* err, int32_t* err_host, int64_t spin, hipStream_t st);
void p2p_gather(const int32_t* inbox, const int32_t* applied, int G, int self, int Q, int64_t H,
                int64_t C, int kw, int nb, int32_t* stage, int32_t* ready, hipStream_t st);
// total may be null
void p2p_commit(int32_t* applied, const int32_t* ready, int G, int64_t* total, hipStream_t st);
// a zeroed fine-grained device buffer (cross-device coherent while kernels run)
void* p2p_fine_alloc(size_t bytes);
void p2p_fine_free(void* p);
// 72-byte handle: the 64-byte IPC handle and the offset of ptr in its allocation
void ipc_export(const void* ptr, uint8_t* out72);
void* ipc_import(const uint8_t* in72);
void ipc_close(void* ptr, int64_t off);

}  // namespace psamd
