// pmmg_graph.hpp — internal interface of pmmg_graph.hip (the METIS element
// graph of a group and its metric weights); the C-ABI wrapper lives in
// pmmg_hip.hip.
#pragma once
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

#include "pmmg_snapshot.hpp"

// Device scratch of the graph passes, owned by a context and kept between
// calls (grown, never shrunk).
struct GraphCache {
  BlockScan rows; // graph entries per block, their offsets
  DevBuf flags;   // the call's flag bits
  DevBuf adja;    // the adjacency of a call that came without one
};

// pmmg_hip_metis_graph on checked arguments.  m.tetv may be NULL without
// weights (every row counts as used); m.adja NULL: built from tetv into the
// cache (pmmg_snap_adjacency, which sets msg when it fails).
// want_wgt 0: adjwgt, xyz and met are not touched.  *nadjncy on the host.
// Synchronous.  Returns 1, or 0 with msg set.
int pmmg_graph_metis(hipStream_t s, int np, const double *xyz, TetView m, int want_wgt, int met_size,
                     const double *met, int cap, int64_t *nadjncy, int *xadj, int *adjncy, int *adjwgt,
                     GraphCache *cache, SnapCache *snap, char *msg, size_t msglen);
