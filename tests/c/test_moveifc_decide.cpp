// The host-side decisions of the interface displacement
// (csrc/pmmg_moveifc_decide.hpp) on a host, built with ASan + UBSan by
// tests/test_moveifc_decide_host.py: the brake of a layer and the packing of
// the colours.
#include <stdio.h>
#include <stdlib.h>

#include <vector>

#include "pmmg_moveifc_decide.hpp"

static int fails = 0;
#define CHECK(x)                                                  \
  do {                                                            \
    if (!(x)) {                                                   \
      printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #x);       \
      fails++;                                                    \
    }                                                             \
  } while (0)

// the reference's counter on `events` events of previous colour g: 1 if it stops before the last
static int loop_brakes(int negrp, int nemin, int events) {
  for (int i = 0; i < events; i++) {
    if (negrp == nemin) return 1;
    negrp--;
  }
  return 0;
}

int main() {
  // the brake against the counter it replaces, on every small (negrp, nemin, D)
  for (int n = 1; n <= 40; n++) {
    const int nemin = n / 2 + 1 < 6 ? n / 2 + 1 : 6;
    for (int d = 0; d <= n + 2; d++) {
      std::vector<int> D{0, d, 0}, nelem{-1, n, 5}, nmin{0, nemin, 3};
      const int g = ifc_first_braked(3, D.data(), nelem.data(), nmin.data());
      CHECK((g == 1) == (loop_brakes(n, nemin, d) == 1));
      CHECK(g == 1 || g == -1);
      if (g < 0) {
        ifc_commit_counts(3, D.data(), nelem.data());
        CHECK(nelem[0] == -1 && nelem[1] == n - d && nelem[2] == 5 && nelem[1] >= nemin);
      }
    }
  }
  { // a colour that is not local never brakes, whatever it loses; the largest counts do not overflow
    std::vector<int> D{2147483647, 2147483647}, nelem{-1, 2147483647}, nmin{0, 6};
    CHECK(ifc_first_braked(2, D.data(), nelem.data(), nmin.data()) == 1);
    nelem[1] = -1;
    CHECK(ifc_first_braked(2, D.data(), nelem.data(), nmin.data()) == -1);
  }
  { // the packing: colours 1, 2, 5 present of 6, the caller's order 4 5 0 1 2 3
    const unsigned char present[6] = {0, 1, 1, 0, 0, 1};
    const int order[6] = {2, 3, 4, 5, 0, 1};
    int map[6];
    CHECK(ifc_pack_colors(6, present, order, map) == 3);
    CHECK(map[5] == 0 && map[1] == 1 && map[2] == 2 && map[0] == -1 && map[3] == -1 && map[4] == -1);
    const int same[6] = {0, 0, 0, 0, 0, 0}; // equal places: the colours' own order
    CHECK(ifc_pack_colors(6, present, same, map) == 3 && map[1] == 0 && map[2] == 1 && map[5] == 2);
    const unsigned char none[1] = {0};
    CHECK(ifc_pack_colors(1, none, same, map) == 0 && map[0] == -1);
  }
  if (!fails) printf("all decided\n");
  return fails ? 1 : 0;
}
