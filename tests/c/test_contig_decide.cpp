// test_contig_decide.cpp — the host-side decision of pmmg_hip_fix_contiguity
// (parmmg_amd/csrc/pmmg_contig_decide.hpp) on tables written out by hand: the
// small graphs of tests/contig_ref.py.  A stand-alone program, built with
// -fsanitize=address,undefined by tests/test_contig_ref_host.py; the arrays
// are heap blocks of exactly the table's length, so that a read or a write
// past a row is an error.
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <vector>

#include "pmmg_contig_decide.hpp"

static int g_checks = 0, g_failed = 0;

#define CHECK(cond)                                                   \
  do {                                                                \
    g_checks++;                                                       \
    if (!(cond)) {                                                    \
      g_failed++;                                                     \
      printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #cond);      \
    }                                                                 \
  } while (0)

struct Run {
  std::vector<int> target;
  ContigCounts n;
  int moved;
};

static Run run(const std::vector<ContigSub> &rows, const std::vector<int> &exitcol, int color, ContigCounts n0 = {}) {
  // exact-size heap copies (the vectors' capacity may exceed their size)
  ContigSub *sub = (ContigSub *)malloc(sizeof(ContigSub) * rows.size());
  int *ec = (int *)malloc(sizeof(int) * rows.size()), *target = (int *)malloc(sizeof(int) * rows.size());
  if (!rows.empty()) {
    memcpy(sub, rows.data(), sizeof(ContigSub) * rows.size());
    memcpy(ec, exitcol.data(), sizeof(int) * rows.size());
  }
  Run r;
  r.n = n0;
  r.moved = contig_decide(sub, ec, (int64_t)rows.size(), color, target, &r.n);
  if (!rows.empty()) r.target.assign(target, target + rows.size());
  free(sub);
  free(ec);
  free(target);
  return r;
}

int main() {
  typedef std::vector<int> V;
  { // the 7-path 0 0 0 1 0 1 1, colour 0: {5} takes colour 1
    std::vector<ContigSub> t = {{0, 1, 3, 13}, {1, 4, 1, 16}, {0, 5, 1, 20}, {1, 6, 2, 24}};
    Run r = run(t, V{1, 0, 1, 0}, 0);
    CHECK(r.target == (V{-1, -1, 1, -1}) && r.moved == 1 && r.n.nmoved == 1 && r.n.nmerged == 1 && r.n.nstuck == 0);
    // ... and colour 1 from the same (stale) table: main {4} is smaller than {6, 7} and leaves
    r = run(t, V{1, 0, 1, 0}, 1);
    CHECK(r.target == (V{-1, 0, -1, -1}) && r.moved == 1 && r.n.nmoved == 1);
  }
  { // equal sizes: main stays the lower head
    std::vector<ContigSub> t = {{0, 1, 2, 9}, {1, 3, 1, 12}, {0, 4, 2, 16}};
    Run r = run(t, V{1, 0, 1}, 0);
    CHECK(r.target == (V{-1, -1, 1}) && r.n.nmoved == 2 && r.n.nmerged == 1);
  }
  { // a stuck main: nothing moves; a later larger one is compared with the old main; a smaller one moves
    std::vector<ContigSub> t = {{0, 1, 2, 0}, {0, 3, 3, 21}, {1, 6, 1, 24}, {0, 7, 3, 28}, {1, 10, 1, 40}, {0, 11, 1, 44}};
    Run r = run(t, V{-1, 1, 0, 1, 0, 1}, 0);
    CHECK(r.target == (V{-1, -1, -1, -1, -1, 1}) && r.n.nstuck == 2 && r.n.nmerged == 1 && r.n.nmoved == 1);
    // the counts add to what they held
    ContigCounts n0;
    n0.nmoved = 1LL << 33;
    n0.nmerged = 5;
    n0.nstuck = 7;
    r = run(t, V{-1, 1, 0, 1, 0, 1}, 0, n0);
    CHECK(r.n.nmoved == (1LL << 33) + 1 && r.n.nmerged == 6 && r.n.nstuck == 9);
  }
  { // a later subgroup without an exit: stuck, main unchanged
    std::vector<ContigSub> t = {{0, 1, 5, 7}, {0, 9, 2, 0}, {0, 20, 9, 81}};
    Run r = run(t, V{1, -1, 2}, 0);
    CHECK(r.target == (V{1, -1, -1}) && r.n.nstuck == 1 && r.n.nmoved == 5); // main {1..} leaves for {20..}
  }
  { // one subgroup, a colour nobody has, an empty table
    std::vector<ContigSub> t = {{0, 1, 3, 0}, {2, 4, 4, 0}};
    Run r = run(t, V{-1, -1}, 0);
    CHECK(r.moved == 0 && r.target == (V{-1, -1}));
    r = run(t, V{-1, -1}, 1);
    CHECK(r.moved == 0 && r.target == (V{-1, -1}) && r.n.nstuck == 0);
    r = run(std::vector<ContigSub>(), V(), 0);
    CHECK(r.moved == 0 && r.target.empty());
  }
  printf("test_contig_decide: %d checks, %d failed\n", g_checks, g_failed);
  return g_failed ? 1 : 0;
}
