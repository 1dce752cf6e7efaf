// pmmg_devbuf.hpp — the one owner of device memory on the host side: every
// hipMalloc'ed block of a context (its work buffers, owned copies, kept
// slots, the scratch caches of pmmg_snapshot / pmmg_meshstats / pmmg_graph)
// is a DevBuf, and goes back to the device when its DevBuf does.
//
// The two allocation calls are macros so that the type can be tested on a
// host without a HIP runtime (tests/c/test_devbuf.cpp): a file that defines
// PMMG_DEV_MALLOC and PMMG_DEV_FREE before including this header also
// declares hipError_t, hipSuccess and hipGetLastError itself.
#pragma once
#include <stddef.h>

#ifndef PMMG_DEV_MALLOC
#include <hip/hip_runtime.h>
#define PMMG_DEV_MALLOC hipMalloc
#define PMMG_DEV_FREE hipFree
#endif

// Move-only {pointer, capacity}; a moved-from buffer is {nullptr, 0}.
struct DevBuf {
  void *p = nullptr;
  size_t cap = 0;

  DevBuf() = default;
  DevBuf(const DevBuf &) = delete;
  DevBuf &operator=(const DevBuf &) = delete;
  DevBuf(DevBuf &&o) noexcept : p(o.p), cap(o.cap) {
    o.p = nullptr;
    o.cap = 0;
  }
  DevBuf &operator=(DevBuf &&o) noexcept {
    if (this != &o) {
      release();
      p = o.p;
      cap = o.cap;
      o.p = nullptr;
      o.cap = 0;
    }
    return *this;
  }
  ~DevBuf() { release(); }

  template <class T> // the block as elements of T (no allocation: nullptr while the buffer is empty)
  T *as() const { return static_cast<T *>(p); }

  void release() {
    if (p) (void)PMMG_DEV_FREE(p);
    p = nullptr;
    cap = 0;
  }

  // At least `bytes` (0 asks for 16); grown, never shrunk, contents not kept:
  // the old block is freed before the new one is allocated.  A failed
  // allocation leaves {nullptr, 0} and clears the runtime's sticky error.
  hipError_t ensure(size_t bytes) {
    if (bytes == 0) bytes = 16;
    if (cap >= bytes) return hipSuccess;
    release();
    const hipError_t e = PMMG_DEV_MALLOC(&p, bytes);
    if (e != hipSuccess) {
      p = nullptr;
      (void)hipGetLastError();
      return e;
    }
    cap = bytes;
    return hipSuccess;
  }
};

// `count` elements of T in b; nullptr when the device has no memory for them
template <class T>
T *get(DevBuf &b, size_t count) {
  return b.ensure(count * sizeof(T)) == hipSuccess ? static_cast<T *>(b.p) : nullptr;
}

// The counts of a count / fill kernel pair: btot[b] of block b, boff[b] the
// sum before it, boff[nblk] the total; tmp is the scan's temporary
// (reserve() and offsets() of pmmg_devutil.hpp).
struct BlockScan {
  DevBuf btot, boff, tmp;
};
