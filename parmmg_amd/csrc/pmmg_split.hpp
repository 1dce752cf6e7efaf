// pmmg_split.hpp — internal interface of pmmg_split.hip (the sub-meshes and
// interface lists of a partition); the C-ABI wrappers live in
// pmmg_hip.hip.
#pragma once
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

#include "parmmg_hip.h"
#include "pmmg_devbuf.hpp"
#include "pmmg_tetview.hpp"

// Device scratch of the split, owned by a context and kept between calls
// (grown, never shrunk).
struct SplitCache {
  DevBuf words;            // the call's flag bits and the rounds' "left" word
  DevBuf iota, skey;       // the sort's values in (1 .. ne) and its keys out (the colours in new order)
  DevBuf sort_tmp;         // keys and values between two digit passes of the sort (ngrp > 256)
  BlockScan digits;        // the sort's (digit, tile) counts and their scan
  DevBuf pos;              // pos[ne]: an old tetra's new place over all groups, 0-based
  DevBuf teoff;            // teoff[ngrp + 1]: the first new place of every colour
  DevBuf first;            // first[4 ne]: per new corner, the corner that uses its vertex first in the group; -1 unsettled
  DevBuf vmin[2];          // per vertex: the lowest (colour, corner) among the corners not settled yet, ping-ponged
  DevBuf nmin;             // per vertex: the lowest (colour, 12 tetra + 3 face + p) over interface faces
  DevBuf vpos;             // per vertex: the position a group gave it in the node list
  DevBuf mask;             // mask[ne]: per new tetra, which corners / faces / face corners make an entry
  DevBuf pre;              // pre[5][ne + 1]: entries before a new tetra, per kind
  BlockScan blocks;        // the five kinds' counts per block, one after the other, and their scan
  DevBuf table;            // table[ngrp + 1]: the counts per group and the totals
  int rounds = 0;          // first-use rounds of the last call (pmmg_hip_split_rounds)
};

// pmmg_hip_split_groups on checked arguments.  Synchronous.  Returns 1, or 0 with msg set.
struct SplitArgs {
  int np;
  TetView m;
  const int *part;
  int ngrp;
  const int *node_pos, *face_old;
  int nnode0, nface0;
  pmmg_hip_split_count *count;
  int64_t pt_cap, face_cap, node_cap;
  int *old_tet, *new_tet, *tetv_out, *adja_out, *tet8_out, *old_pt;
  int *face_idx1, *face_idx2, *node_idx1, *node_idx2;
  int *nnode_end, *nface_end;
};
int pmmg_split_groups(hipStream_t s, const SplitArgs &a, SplitCache *cache, char *msg, size_t msglen);
