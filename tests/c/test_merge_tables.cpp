// The host-built tables of pmmg_hip_merge_groups (csrc/pmmg_merge_tables.hpp) on a host without a HIP runtime:
// the four offset tables with empty groups, the colours, the refusals at the limits.  Built with ASan + UBSan by
// tests/test_merge_ref_host.py.
#include <limits.h>
#include <stdio.h>
#include <string.h>

#include <vector>

#include "pmmg_merge_tables.hpp"

static int failed = 0;
#define CHECK(cond)                                             \
  do {                                                          \
    if (!(cond)) {                                              \
      printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #cond);  \
      failed++;                                                 \
    }                                                           \
  } while (0)

int main() {
  char msg[256] = "";
  std::vector<int> tab;
  MergeTotals tot;
  { // empty groups first, in the middle and last
    const pmmg_hip_split_count count[5] = {{0, 0, 0, 0}, {2, 5, 1, 3}, {0, 0, 0, 0}, {3, 6, 2, 1}, {0, 0, 0, 0}};
    const int color[5] = {7, 8, 9, 10, 11};
    CHECK(merge_tables(5, count, color, &tab, &tot, msg, sizeof(msg)) == 1);
    CHECK(tab.size() == 4 * 6 + 5);
    const int te[6] = {0, 0, 2, 2, 5, 5}, pt[6] = {0, 0, 5, 5, 11, 11}, fa[6] = {0, 0, 1, 1, 3, 3}, no[6] = {0, 0, 3, 3, 4, 4};
    CHECK(memcmp(tab.data(), te, sizeof(te)) == 0);
    CHECK(memcmp(tab.data() + 6, pt, sizeof(pt)) == 0);
    CHECK(memcmp(tab.data() + 12, fa, sizeof(fa)) == 0);
    CHECK(memcmp(tab.data() + 18, no, sizeof(no)) == 0);
    CHECK(memcmp(tab.data() + 24, color, sizeof(color)) == 0);
    CHECK(tot.ne == 5 && tot.np == 11 && tot.nface == 3 && tot.nnode == 4);
    // without colours: zeros
    CHECK(merge_tables(5, count, nullptr, &tab, &tot, msg, sizeof(msg)) == 1);
    for (int g = 0; g < 5; g++) CHECK(tab[24 + g] == 0);
  }
  { // one group
    const pmmg_hip_split_count count[1] = {{1, 4, 0, 0}};
    CHECK(merge_tables(1, count, nullptr, &tab, &tot, msg, sizeof(msg)) == 1);
    CHECK(tab.size() == 9 && tab[1] == 1 && tab[3] == 4 && tot.ne == 1 && tot.np == 4);
  }
  { // a negative count
    const pmmg_hip_split_count count[2] = {{1, 4, 0, 0}, {1, -4, 0, 0}};
    CHECK(merge_tables(2, count, nullptr, &tab, &tot, msg, sizeof(msg)) == 0);
    CHECK(strstr(msg, "negative") != nullptr);
  }
  { // the tetra limit: the sum one below it passes, the limit itself does not; the sums do not wrap an int
    pmmg_hip_split_count count[3] = {{kMergeTetMax - 2, 1, 0, 0}, {1, 1, 0, 0}, {0, 0, 0, 0}};
    CHECK(merge_tables(3, count, nullptr, &tab, &tot, msg, sizeof(msg)) == 1);
    CHECK(tot.ne == kMergeTetMax - 1 && 12LL * tot.ne + 11 <= INT_MAX);
    count[2].ne = 1;
    CHECK(merge_tables(3, count, nullptr, &tab, &tot, msg, sizeof(msg)) == 0);
    CHECK(strstr(msg, "12*ie+11") != nullptr);
    const pmmg_hip_split_count wide[3] = {{0, INT_MAX, 0, 0}, {0, INT_MAX, 0, 0}, {0, 2, 0, 0}};
    CHECK(merge_tables(3, wide, nullptr, &tab, &tot, msg, sizeof(msg)) == 0);
    CHECK(strstr(msg, "points") != nullptr);
    const pmmg_hip_split_count lists[1] = {{0, 0, 0, kMergeLenMax}};
    CHECK(merge_tables(1, lists, nullptr, &tab, &tot, msg, sizeof(msg)) == 0);
    CHECK(strstr(msg, "node entries") != nullptr);
  }
  printf("%d failed\n", failed);
  return failed ? 1 : 0;
}
