// pmmg_moveifc_decide.hpp — the two host-side decisions of the interface
// displacement (pmmg_moveifc.hip), without a HIP type: tested
// on a host by tests/c/test_moveifc_decide.cpp.
#pragma once
#include <algorithm>
#include <vector>

// The brake of PMMG_mark_boulevolp over a whole layer.  D[g]: the layer's
// events whose previous colour is g, computed as if nothing braked.  nelem[g]:
// the reference's negrp (-1: the colour is not local and never brakes),
// nemin[g] its floor.  The loop decrements negrp[g] once per event and stops
// at negrp[g] == nemin[g]: no brake fires in the layer iff D[g] <= nelem[g] -
// nemin[g] for every local g that has an event.  Returns the first colour
// that would brake, or -1.
static inline int ifc_first_braked(int ncolor, const int *D, const int *nelem, const int *nemin) {
  for (int g = 0; g < ncolor; g++)
    if (nelem[g] >= 0 && D[g] > 0 && (long long)D[g] > (long long)nelem[g] - nemin[g]) return g;
  return -1;
}

// nelem[g] -= D[g] for the local colours (the layer is committed)
static inline void ifc_commit_counts(int ncolor, const int *D, int *nelem) {
  for (int g = 0; g < ncolor; g++)
    if (nelem[g] >= 0) nelem[g] -= D[g];
}

// The packing of PMMG_part_getInterfaces: the colours present get 0, 1, ...
// in ascending (order[c], c); map[c] = -1 for a colour that is absent.
// Returns the number of colours present.
static inline int ifc_pack_colors(int ncolor, const unsigned char *present, const int *order, int *map) {
  std::vector<int> cols;
  for (int c = 0; c < ncolor; c++) {
    map[c] = -1;
    if (present[c]) cols.push_back(c);
  }
  std::stable_sort(cols.begin(), cols.end(), [&](int a, int b) { return order[a] < order[b]; });
  for (size_t i = 0; i < cols.size(); i++) map[cols[i]] = (int)i;
  return (int)cols.size();
}
