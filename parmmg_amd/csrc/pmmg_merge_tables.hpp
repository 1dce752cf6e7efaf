// pmmg_merge_tables.hpp — the host-built tables of pmmg_hip_merge_groups: the four offset
// tables of the concatenated groups and the colours, in the one int array that the call uploads.  No HIP
// type, so it is tested on a host: tests/c/test_merge_tables.cpp.
#pragma once
#include <stdint.h>
#include <stdio.h>

#include <vector>

#include "parmmg_hip.h"

// 12 * ie + 11 stays an int for a merged tetra ie below this (the reference's intvalues have the same limit)
constexpr int kMergeTetMax = 178956970;
// the other lengths: an index plus a grid's stride stays an int
constexpr int kMergeLenMax = 1 << 29;

// The lengths of the concatenated arrays.
struct MergeTotals { int ne, np, nface, nnode; };

// tab = te_off | pt_off | face_off | node_off (ngrp + 1 entries each, exclusive prefix sums of count[].ne,
// .np, .nface, .nnode) | color (ngrp entries, zeros without colours).  Returns 1, or 0 with msg set: a
// negative count, or a total beyond its limit.
static inline int merge_tables(int ngrp, const pmmg_hip_split_count *count, const int *color, std::vector<int> *tab,
                               MergeTotals *tot, char *msg, size_t msglen) {
  const size_t G = (size_t)ngrp + 1;
  tab->assign(4 * G + (size_t)ngrp, 0);
  int64_t at[4] = {0, 0, 0, 0};
  for (int g = 0; g < ngrp; g++) {
    const int c[4] = {count[g].ne, count[g].np, count[g].nface, count[g].nnode};
    for (int i = 0; i < 4; i++) {
      if (c[i] < 0) {
        snprintf(msg, msglen, "merge_groups: invalid arguments (a negative count in group %d)", g);
        return 0;
      }
      at[i] += c[i];
      if (at[i] >= (i == 0 ? kMergeTetMax : kMergeLenMax)) {
        if (i == 0)
          snprintf(msg, msglen, "merge_groups: the groups' tetra reach %d: 12*ie+11 must fit an int (nothing written)",
                   kMergeTetMax);
        else
          snprintf(msg, msglen, "merge_groups: the groups' %s reach 2^29 (nothing written)",
                   i == 1 ? "points" : (i == 2 ? "face entries" : "node entries"));
        return 0;
      }
      (*tab)[i * G + g + 1] = (int)at[i];
    }
    if (color) (*tab)[4 * G + g] = color[g];
  }
  *tot = MergeTotals{(int)at[0], (int)at[1], (int)at[2], (int)at[3]};
  return 1;
}
