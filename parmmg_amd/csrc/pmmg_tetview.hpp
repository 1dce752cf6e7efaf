// pmmg_tetview.hpp — the tetra rows of a mesh service call, and the one place
// that decodes them from an entry point's (ne, tetv, adja, tet8).  No HIP type
// and no error text (an entry point of pmmg_hip.hip turns the code into its
// own message), so it is tested on a host: tests/c/test_tetview.cpp.
#pragma once
#include <stdint.h>

// Tetra rows as int4 rows `tstride` / `astride` int4s apart (1: separate
// arrays, 2: the packed {v[4], adja[4]} records of tet8).  Which of the two
// arrays may be NULL is the service's own rule (pmmg_snapshot.hpp,
// pmmg_graph.hpp, pmmg_contig.hpp).
struct TetView { int ne; const int *tetv; int tstride; const int *adja; int astride; };

// a link 4 k + i with k <= ne stays an int below this many tetra
constexpr int kTetMax = 1 << 29;

template <int N>
static inline bool aligned(const void *p) {
  return ((uintptr_t)p & (uintptr_t)(N - 1)) == 0;
}

enum TetArgs { TET_OK = 0, TET_MISSING, TET_TOOMANY, TET_MISALIGNED };
// what a caller asks of separate arrays (tet8 has both); neither bit: one of the two is enough
enum { TET_NEED_TETV = 1, TET_NEED_ADJA = 2, TET_ANY_NE = 4 /* no kTetMax bound */ };

// *v from the arguments of an entry point, tet8 winning over tetv / adja, and
// the first of: an array the caller needs is NULL, ne >= kTetMax, a base that
// is not 16-byte aligned (NULL is).  A mesh of ne <= 0 has no rows to check.
static inline TetArgs tet_view(int ne, const int *tetv, const int *adja, const int *tet8, int need, TetView *v) {
  const int stride = tet8 ? 2 : 1;
  *v = TetView{ne, tet8 ? tet8 : tetv, stride, tet8 ? tet8 + 4 : adja, stride};
  if (ne <= 0) return TET_OK;
  if ((!v->tetv && ((need & TET_NEED_TETV) || !v->adja)) || (!v->adja && (need & TET_NEED_ADJA))) return TET_MISSING;
  if (ne >= kTetMax && !(need & TET_ANY_NE)) return TET_TOOMANY;
  if (!aligned<16>(v->tetv) || !aligned<16>(v->adja)) return TET_MISALIGNED;
  return TET_OK;
}
