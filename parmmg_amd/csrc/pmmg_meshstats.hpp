// pmmg_meshstats.hpp — internal interface of pmmg_meshstats.hip (quality and
// edge-length reports of the adapted mesh); the C-ABI wrappers live in
// pmmg_hip.hip.
#pragma once
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

#include "parmmg_hip.h"
#include "pmmg_devbuf.hpp"

// Device scratch of the two reports, owned by a context and kept between
// calls (grown, never shrunk): the edge table, the ownership bytes, the
// per-block slabs.
struct StatsCache {
  DevBuf keys, own;  // the edge table: keys and owner codes
  DevBuf small;      // 32 counters, then the 2 flags
  DevBuf slab, mask; // per-block partials; the tetra's owned-edge bits
  DevBuf res;        // the report on the device
  BlockScan list;    // list pass: analysed edges per block, their offsets
  // the table size a call had to grow to, and the counts it was for: the next call on such a mesh starts there
  long long grown_nslot = 0;
  int grown_np = 0, grown_ne = 0, grown_nskip = 0, grown_mode = 0;
};
int64_t pmmg_stats_cache_bytes(const StatsCache *c);

// pmmg_hip_qual_histo: device pointers (tetv 16-byte aligned), *out on the
// host.  Synchronous.  Returns 1, or 0 with msg set.
int pmmg_stats_qual_histo(hipStream_t s, int ne, const int *tetv, const double *qual, pmmg_hip_qual_histo_t *out,
                          StatsCache *cache, char *msg, size_t msglen);

// pmmg_hip_edge_lengths.  hash_mode 0: the table slot is a mix of the whole
// key; 1: a run of slots per low vertex first (the edges of one low vertex
// share a few neighbouring lines), then stepped from the mix.  Same results
// either way.
int pmmg_stats_edge_lengths(hipStream_t s, int np, const double *xyz, int ne, const int *tetv, int met_size,
                            const double *met, int nskip, const int *skip, pmmg_hip_len_histo_t *out, int cap,
                            int *edge_out, double *len_out, int hash_mode, StatsCache *cache, char *msg,
                            size_t msglen);
