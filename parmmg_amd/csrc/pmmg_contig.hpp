// pmmg_contig.hpp — internal interface of pmmg_contig.hip (the subgroups of a
// partition and their fix); the C-ABI wrappers live in
// pmmg_hip.hip.
#pragma once
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

#include "parmmg_hip.h"
#include "pmmg_snapshot.hpp"

// Device scratch of the contiguity passes, owned by a context and kept
// between calls (grown, never shrunk).
struct ContigCache {
  DevBuf parent;           // P[ne]: a tetra's parent (-1: unused); the hooks of a round go here
  DevBuf label;            // L[ne]: a tetra's root at the start of a round, after a labelling its subgroup's lowest tetra
  DevBuf idx;              // idx[ne]: at a head, its row in the table
  BlockScan heads;         // heads per block, their offsets
  DevBuf words;            // the call's flag bits, the passes' "changed" / "unfinished" words, the vertex maximum
  DevBuf sub, exitcol;     // the table and, per row, the colour across its exit
  DevBuf rank;             // per row: flag's value (part_subgroups) or the colour it takes (fix_contiguity)
  DevBuf adja;             // the adjacency of a call that came without one
  int64_t passes = 0;      // flatten passes of the last call (pmmg_hip_contig_passes)
};

// pmmg_hip_part_subgroups / pmmg_hip_fix_contiguity on checked arguments:
// m.tetv may be NULL (every row is used); m.adja NULL: built from tetv into
// the cache; part NULL: one colour.  Synchronous.  Return 1, or 0 with msg set.
int pmmg_contig_subgroups(hipStream_t s, TetView m, const int *part, int ncolor, int *head, int *flag, int *ncomp,
                          int cap, pmmg_hip_subgroup *sub, int64_t *nsub, int *rounds, ContigCache *cache,
                          SnapCache *snap, char *msg, size_t msglen);
int pmmg_contig_fix(hipStream_t s, TetView m, int *part, int ncolor, int64_t *nmoved, int *nmerged, int *nstuck,
                    ContigCache *cache, SnapCache *snap, char *msg, size_t msglen);
