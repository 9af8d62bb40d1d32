// Host-side geometry shared by the units of the "tp" / "tpf" kernel family (internal: the
// public launchers are in tploc.h). tp_geom, tp_flat_lts and tp_launch_tile are defined
// in tploc.hip, tpf_launch_bucket in tploc_bucket.hip.
#pragma once
#include "tploc.h"

namespace psamd {

struct TpGeom {
  int nbk, shift;
  int lts;      // log2 occurrences per tile
  int64_t T, N;  // tiles, entry stride (T * kTile)
};

int tp_flat_lts(int64_t n);  // log2 occurrences per tile of the flat layout
TpGeom tp_geom(int64_t n, int bits, bool flat = false);

// flat layout: bucket workgroups take pairs of fine buckets where the geometry allows
inline bool tpf_pair(const TpGeom& g) { return g.nbk >= 2 && g.shift <= 30; }
inline int tpf_groups_of(const TpGeom& g) { return tpf_pair(g) ? g.nbk / 2 : g.nbk; }

inline size_t al16(size_t x) { return (x + 15) & ~(size_t)15; }

// The tile kernel of either layout: tp_tile_kernel<kQuot, kCnt> with kQuot = keys above
// 31 bits (quotient-encoded hash), kCnt = ecnt != null (the tail filter's per-entry
// occurrence counts).
void tp_launch_tile(const uint64_t* raw, int64_t n, KeyMix m, const TpGeom& g, uint32_t* tkeys,
                    uint16_t* toff, int32_t* dcnt, uint16_t* rep, int32_t* err, uint8_t* ecnt,
                    hipStream_t st);
// The flat layout's bucket kernel (tploc_bucket.hip): tpf_bucket_kernel<kFilt> with
// kFilt = ecnt != null (the keys carry their occurrence counts for the tail filter).
void tpf_launch_bucket(const TpGeom& g, const uint32_t* tkeys, const uint16_t* toff,
                       uint64_t* uniqf, int32_t* ent_pos, uint16_t* ent_j, int32_t* cnt,
                       int32_t* err, bool sorted, const uint8_t* ecnt, hipStream_t st);

}  // namespace psamd
