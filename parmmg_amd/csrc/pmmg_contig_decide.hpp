// pmmg_contig_decide.hpp — the host-side decision of pmmg_hip_fix_contiguity
// for one colour: PMMG_fix_subgrp_contiguity's comparison of
// every later subgroup with the main one (reference
// src/moveinterfaces_pmmg.c:377-465), on the subgroup table the device
// produced.  Plain C++ without a HIP runtime, so that tests/c/test_contig_decide.cpp
// can drive it on a host under the sanitizers.
#pragma once
#include <stdint.h>

// One row of the table: pmmg_hip_subgroup's fields (include/parmmg_hip.h).
struct ContigSub {
  int color, head, size, exit;
};

struct ContigCounts {
  int64_t nmoved = 0; // tetra of the moved subgroups
  int nmerged = 0;    // moved subgroups
  int nstuck = 0;     // subgroups that should have moved and touch no other colour
};

// The subgroups of `color` among sub[0 .. nsub) (ascending head), exitcol[i] =
// the colour of the tetra across sub[i].exit (unspecified where exit == 0).
// target[i] receives the colour subgroup i takes, or -1 where it keeps its
// own (every row of another colour).  Returns the number of moved subgroups
// and adds to *n.
//   main = the first; for every later one, next:
//     next.size > main.size:  main has an exit -> main moves, next is main;
//                             else nothing moves, main stays, nstuck++
//     otherwise:              next has an exit -> next moves; else nstuck++
static inline int contig_decide(const ContigSub *sub, const int *exitcol, int64_t nsub, int color, int *target,
                                ContigCounts *n) {
  int64_t main_i = -1;
  int moved = 0;
  for (int64_t i = 0; i < nsub; i++) {
    target[i] = -1;
    if (sub[i].color != color) continue;
    if (main_i < 0) {
      main_i = i;
      continue;
    }
    int64_t out = i; // the subgroup that leaves the colour
    if (sub[i].size > sub[main_i].size) {
      if (sub[main_i].exit == 0) {
        n->nstuck++;
        continue;
      }
      out = main_i;
      main_i = i;
    } else if (sub[i].exit == 0) {
      n->nstuck++;
      continue;
    }
    target[out] = exitcol[out];
    n->nmoved += sub[out].size;
    n->nmerged++;
    moved++;
  }
  return moved;
}
