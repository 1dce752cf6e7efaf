// tet_view (csrc/pmmg_tetview.hpp), the decode-and-check of an entry point's
// (ne, tetv, adja, tet8), on a host: every pointer is a fabricated integer
// and none is dereferenced.  Built with ASan + UBSan by
// tests/test_tetview_host.py.
#include <stdint.h>
#include <stdio.h>

#include <initializer_list>

#include "pmmg_tetview.hpp"

static int g_fail = 0;

static const int *ptr(uintptr_t a) { return reinterpret_cast<const int *>(a); }

// tet_view gives `want` and, whatever the code, the view of the arguments
static void expect(const char *what, int ne, uintptr_t tetv, uintptr_t adja, uintptr_t tet8, int need, TetArgs want) {
  TetView v{-1, ptr(1), -1, ptr(1), -1};
  const TetArgs got = tet_view(ne, ptr(tetv), ptr(adja), ptr(tet8), need, &v);
  const uintptr_t t0 = tet8 ? tet8 : tetv, a0 = tet8 ? tet8 + 4 * sizeof(int) : adja;
  const int stride = tet8 ? 2 : 1;
  const bool view_ok = v.ne == ne && (uintptr_t)v.tetv == t0 && (uintptr_t)v.adja == a0 && v.tstride == stride &&
                       v.astride == stride;
  if (got != want || !view_ok) {
    g_fail++;
    printf("FAIL %s (ne=%d tetv=%#lx adja=%#lx tet8=%#lx need=%d): code %d, expected %d; view {%d, %#lx, %d, %#lx, %d}\n",
           what, ne, (unsigned long)tetv, (unsigned long)adja, (unsigned long)tet8, need, (int)got, (int)want, v.ne,
           (unsigned long)(uintptr_t)v.tetv, v.tstride, (unsigned long)(uintptr_t)v.adja, v.astride);
  }
}

int main() {
  const uintptr_t T = 0x10000, A = 0x20000, P = 0x30000; // 16-byte lines
  // the callers' policies: metis_graph without / with weights, the contiguity calls, build_boundary
  const int kGraph = 0, kGraphW = TET_NEED_TETV, kContig = 0, kBdy = TET_NEED_TETV | TET_NEED_ADJA | TET_ANY_NE;
  const int policy[4] = {kGraph, kGraphW, kContig, kBdy};

  static_assert(kTetMax == (1 << 29), "the bound of the 4 k + i encoding");

  for (int need : policy) {
    // packed against separate arrays: strides 2 and 1, adja == tet8 + 4 (checked by expect on every case)
    expect("separate", 6, T, A, 0, need, TET_OK);
    expect("packed", 6, 0, 0, P, need, TET_OK);
    expect("packed wins over separate", 6, T, A, P, need, TET_OK);
    expect("packed wins over misaligned separate", 6, T + 4, A + 8, P, need, TET_OK);

    // each array NULL in turn
    const bool need_t = need & TET_NEED_TETV, need_a = need & TET_NEED_ADJA;
    expect("tetv NULL", 6, 0, A, 0, need, need_t ? TET_MISSING : TET_OK);
    expect("adja NULL", 6, T, 0, 0, need, need_a ? TET_MISSING : TET_OK);
    expect("both NULL", 6, 0, 0, 0, need, TET_MISSING);
    expect("both NULL, no rows", 0, 0, 0, 0, need, TET_OK);

    // ne = 0, 1, 2^29 - 1, 2^29
    const TetArgs big = (need & TET_ANY_NE) ? TET_OK : TET_TOOMANY;
    expect("ne 0", 0, T, A, 0, need, TET_OK);
    expect("ne 1", 1, T, A, 0, need, TET_OK);
    expect("ne 2^29 - 1", kTetMax - 1, T, A, 0, need, TET_OK);
    expect("ne 2^29", kTetMax, T, A, 0, need, big);
    expect("ne 2^29 packed", kTetMax, 0, 0, P, need, big);
    expect("ne INT_MAX", 0x7fffffff, T, A, 0, need, big);
    // the order of the refusals: a missing array first, then the bound, then the alignment
    expect("ne 2^29, both NULL", kTetMax, 0, 0, 0, need, TET_MISSING);
    expect("ne 2^29, misaligned", kTetMax, T + 4, A, 0, need, (need & TET_ANY_NE) ? TET_MISALIGNED : TET_TOOMANY);

    // every base at +4 and +8 from a 16-byte line
    for (uintptr_t d : {(uintptr_t)4, (uintptr_t)8}) {
      expect("tetv off a line", 6, T + d, A, 0, need, TET_MISALIGNED);
      expect("adja off a line", 6, T, A + d, 0, need, TET_MISALIGNED);
      expect("tet8 off a line", 6, 0, 0, P + d, need, TET_MISALIGNED);
      expect("tetv off a line, adja NULL", 6, T + d, 0, 0, need, need_a ? TET_MISSING : TET_MISALIGNED);
      expect("adja off a line, tetv NULL", 6, 0, A + d, 0, need, need_t ? TET_MISSING : TET_MISALIGNED);
      expect("off a line, no rows", 0, T + d, A + d, 0, need, TET_OK); // (a mesh without rows is not looked at)
      expect("packed off a line, no rows", 0, 0, 0, P + d, need, TET_OK);
    }
  }

  // aligned<N>: NULL is aligned; the bits below N decide
  if (!aligned<16>(ptr(0)) || !aligned<16>(ptr(T)) || aligned<16>(ptr(T + 8)) || !aligned<8>(ptr(T + 8)) ||
      aligned<8>(ptr(T + 4)) || !aligned<4>(ptr(T + 4)) || aligned<4>(ptr(T + 2))) {
    g_fail++;
    printf("FAIL aligned<N>\n");
  }

  if (g_fail) {
    printf("%d case(s) failed\n", g_fail);
    return 1;
  }
  printf("all views as expected\n");
  return 0;
}
