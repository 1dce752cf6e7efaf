// test_devbuf.cpp — DevBuf (parmmg_amd/csrc/pmmg_devbuf.hpp) on a host
// without a HIP runtime: the two allocation calls are replaced by a stub that
// counts live blocks and bytes and can make the next allocation fail.  Built
// with -fsanitize=address,undefined by tests/test_devbuf_host.py; every case
// ends with nothing live, so a buffer that is dropped without being freed
// (a shrinking vector of the old plain struct) fails here.
#include <stddef.h>
#include <stdio.h>
#include <stdlib.h>

#include <map>
#include <utility>
#include <vector>

typedef int hipError_t;
static const hipError_t hipSuccess = 0, hipErrorOutOfMemory = 2;

static std::map<void *, size_t> g_live; // block -> bytes
static size_t g_live_bytes = 0, g_last_bytes = 0;
static int g_mallocs = 0, g_frees = 0, g_fail_next = 0, g_sticky = 0;
static bool g_overlap = false; // an allocation made while another block of the watched buffer was live
static bool g_watch = false;

static hipError_t stub_malloc(void **p, size_t bytes) {
  if (g_fail_next) {
    g_fail_next = 0;
    g_sticky = 1;
    *p = (void *)0x1; // what a failed call left behind must not be kept
    return hipErrorOutOfMemory;
  }
  if (g_watch && !g_live.empty()) g_overlap = true;
  *p = malloc(bytes);
  g_live[*p] = bytes;
  g_live_bytes += bytes;
  g_last_bytes = bytes;
  g_mallocs++;
  return hipSuccess;
}
static hipError_t stub_free(void *p) {
  std::map<void *, size_t>::iterator it = g_live.find(p);
  if (it == g_live.end()) {
    fprintf(stderr, "FAIL: free of a block that is not live (%p)\n", p);
    exit(1);
  }
  g_live_bytes -= it->second;
  g_live.erase(it);
  free(p);
  g_frees++;
  return hipSuccess;
}
static hipError_t hipGetLastError() {
  const hipError_t e = g_sticky ? hipErrorOutOfMemory : hipSuccess;
  g_sticky = 0;
  return e;
}

#define PMMG_DEV_MALLOC stub_malloc
#define PMMG_DEV_FREE stub_free
#include "pmmg_devbuf.hpp"

static int g_checks = 0;
#define CHECK(cond)                                                        \
  do {                                                                     \
    g_checks++;                                                            \
    if (!(cond)) {                                                         \
      fprintf(stderr, "FAIL %s:%d: %s\n", __FILE__, __LINE__, #cond);      \
      exit(1);                                                             \
    }                                                                      \
  } while (0)

// every case starts and ends with nothing live
#define NOTHING_LIVE() CHECK(g_live.empty() && g_live_bytes == 0)

static void case_ensure() {
  {
    DevBuf b;
    CHECK(b.p == nullptr && b.cap == 0);
    CHECK(b.ensure(0) == hipSuccess);
    CHECK(b.p && b.cap == 16 && g_last_bytes == 16 && g_live.size() == 1 && g_live_bytes == 16);
    void *p0 = b.p;
    const int m0 = g_mallocs, f0 = g_frees;
    CHECK(b.ensure(16) == hipSuccess && b.ensure(7) == hipSuccess && b.ensure(0) == hipSuccess);
    CHECK(b.p == p0 && b.cap == 16 && g_mallocs == m0 && g_frees == f0); // n <= cap: nothing allocated
    g_watch = true; // growth: the old block goes before the new one comes
    CHECK(b.ensure(1000) == hipSuccess);
    g_watch = false;
    CHECK(!g_overlap && g_mallocs == m0 + 1 && g_frees == f0 + 1);
    CHECK(b.cap == 1000 && g_live.size() == 1 && g_live_bytes == 1000 && g_live.count(b.p) == 1);
    CHECK(get<double>(b, 125) == b.p && g_mallocs == m0 + 1); // 1000 bytes: fits
    double *d = get<double>(b, 126);
    CHECK(d && d == b.p && b.cap == 1008 && g_live_bytes == 1008);
    b.release();
    CHECK(b.p == nullptr && b.cap == 0);
    NOTHING_LIVE();
    b.release(); // twice is harmless
    CHECK(b.ensure(32) == hipSuccess && g_live_bytes == 32);
  } // the destructor frees
  NOTHING_LIVE();
}

static void case_failed_allocation() {
  {
    DevBuf b;
    CHECK(b.ensure(64) == hipSuccess);
    g_fail_next = 1;
    CHECK(b.ensure(128) != hipSuccess);
    CHECK(b.p == nullptr && b.cap == 0); // the old block is gone, nothing half-owned
    CHECK(g_sticky == 0);                // the sticky error was cleared
    NOTHING_LIVE();
    g_fail_next = 1;
    CHECK(get<int>(b, 8) == nullptr && b.p == nullptr && b.cap == 0);
    CHECK(b.ensure(128) == hipSuccess && b.p && b.cap == 128 && g_live_bytes == 128); // a later ensure succeeds
  }
  NOTHING_LIVE();
}

static void case_move() {
  {
    DevBuf a;
    CHECK(a.ensure(100) == hipSuccess);
    void *pa = a.p;
    const int f0 = g_frees;
    DevBuf b(std::move(a)); // move construction: the source is left empty, nothing freed
    CHECK(a.p == nullptr && a.cap == 0 && b.p == pa && b.cap == 100 && g_frees == f0 && g_live.size() == 1);
    DevBuf c;
    CHECK(c.ensure(50) == hipSuccess);
    void *pc = c.p;
    c = std::move(b); // move assignment: the target's old block is freed
    CHECK(g_frees == f0 + 1 && g_live.count(pc) == 0 && g_live.count(pa) == 1);
    CHECK(b.p == nullptr && b.cap == 0 && c.p == pa && c.cap == 100 && g_live_bytes == 100);
    DevBuf &r = c;
    c = std::move(r); // self-move is harmless
    CHECK(c.p == pa && c.cap == 100 && g_frees == f0 + 1 && g_live_bytes == 100);
    c = DevBuf{}; // an empty source frees the target
    CHECK(c.p == nullptr && c.cap == 0);
    NOTHING_LIVE();
  }
  NOTHING_LIVE();
}

static void case_swap() {
  {
    DevBuf a, b, e;
    CHECK(a.ensure(10) == hipSuccess && b.ensure(20) == hipSuccess);
    void *pa = a.p, *pb = b.p;
    const int m0 = g_mallocs, f0 = g_frees;
    std::swap(a, b);
    CHECK(a.p == pb && a.cap == 20 && b.p == pa && b.cap == 10);
    std::swap(a, e); // with an empty one (pmmg_hip_keep: a staging buffer into an unused slot)
    CHECK(a.p == nullptr && a.cap == 0 && e.p == pb && e.cap == 20);
    CHECK(g_mallocs == m0 && g_frees == f0 && g_live.size() == 2 && g_live_bytes == 30); // nothing freed
  }
  NOTHING_LIVE();
}

static void case_vector() {
  {
    std::vector<DevBuf> v(3);
    for (size_t j = 0; j < v.size(); j++) CHECK(v[j].ensure(8 * (j + 1)) == hipSuccess);
    CHECK(g_live.size() == 3 && g_live_bytes == 8 + 16 + 24);
    void *p0 = v[0].p;
    const int f0 = g_frees;
    v.resize(1); // three fields, then one: the two dropped blocks are freed
    CHECK(g_frees == f0 + 2 && g_live.size() == 1 && g_live_bytes == 8 && v[0].p == p0);
    v.shrink_to_fit();
    v.resize(3); // (reallocates the vector: the elements are moved, not copied)
    CHECK(v[0].p == p0 && v[0].cap == 8 && v[1].p == nullptr && v[2].p == nullptr && g_frees == f0 + 2);
    CHECK(v[1].ensure(40) == hipSuccess && v[2].ensure(48) == hipSuccess && g_live_bytes == 96);
    v.clear();
    NOTHING_LIVE();
    v.resize(2);
    CHECK(v[0].ensure(1) == hipSuccess && v[1].ensure(2) == hipSuccess && g_live.size() == 2);
  } // destruction frees the rest
  NOTHING_LIVE();
  {
    // a struct of buffers and vectors reset by move assignment (a kept slot dropped, a context's teardown)
    struct Kept {
      DevBuf xyz, met;
      std::vector<DevBuf> f;
    };
    Kept k;
    k.f.resize(2);
    CHECK(k.xyz.ensure(24) == hipSuccess && k.met.ensure(48) == hipSuccess && k.f[0].ensure(8) == hipSuccess &&
          k.f[1].ensure(8) == hipSuccess && g_live.size() == 4);
    k = Kept{};
    CHECK(k.xyz.p == nullptr && k.f.empty());
    NOTHING_LIVE();
  }
  NOTHING_LIVE();
}

int main() {
  case_ensure();
  case_failed_allocation();
  case_move();
  case_swap();
  case_vector();
  CHECK(g_mallocs == g_frees);
  printf("test_devbuf: %d checks, %d allocations, all freed\n", g_checks, g_mallocs);
  return 0;
}
