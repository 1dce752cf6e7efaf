// pmmg_merge.hpp — internal interface of pmmg_merge.hip (the groups of a rank
// joined into one mesh); the C-ABI wrappers live in
// pmmg_hip.hip.
#pragma once
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

#include "parmmg_hip.h"
#include "pmmg_devbuf.hpp"

// Device scratch of the merge, owned by a context and kept between calls
// (grown, never shrunk).
struct MergeCache {
  DevBuf words;     // the call's flag bits
  DevBuf tab;       // the four offset tables [ngrp + 1] and the colours [ngrp] (pmmg_merge_tables.hpp)
  DevBuf firsts;    // lowest entries: per point, per tetra, per node position, per face position
  DevBuf counts;    // per node position the groups >= 1 that hold it, per face position their entries
  DevBuf pre;       // the four exclusive prefixes: created points, unlisted points, first face entries, internal tetra
  BlockScan blocks; // the four kinds' counts per block, one after the other, and their scan
};

// pmmg_hip_merge_groups on checked arguments (every pointer the sizes need is there and aligned).
// Synchronous.  Returns 1, or 0 with msg set.
struct MergeArgs {
  int ngrp;
  const pmmg_hip_split_count *count;
  const int *tetv;
  int tstride; // int4s between two rows: 1, or 2 for tet8 records
  const int *node_idx1, *node_idx2, *face_idx1, *face_idx2;
  int nnode, nface;
  const int *color;
  int64_t pt_cap;
  int *new_pt, *new_tet, *src_pt, *src_tet, *tetv_out, *mark_out, *node_val, *face_val;
  int *np_out, *ne_out;
};
int pmmg_merge_groups(hipStream_t s, const MergeArgs &a, MergeCache *cache, char *msg, size_t msglen);
