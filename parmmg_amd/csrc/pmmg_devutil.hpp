// pmmg_devutil.hpp — what the host sides of pmmg_snapshot.hip,
// pmmg_meshstats.hip and pmmg_graph.hip share: the error macro of a function
// that reports through (msg, msglen) and returns 0, and the exclusive scan of
// an int array with its temporary in a DevBuf.
#pragma once
#include <hip/hip_runtime.h>
#include <hipcub/hipcub.hpp>

#include <stdio.h>

#include "pmmg_devbuf.hpp"

#define DEVCK(expr)                                                                                 \
  do {                                                                                              \
    hipError_t e_ = (expr);                                                                         \
    if (e_ != hipSuccess) {                                                                         \
      snprintf(msg, msglen, "%s failed: %s (%s:%d)", #expr, hipGetErrorString(e_), __FILE__, __LINE__); \
      return 0;                                                                                     \
    }                                                                                               \
  } while (0)

// The scan's temporary sized and tmp grown to it, nothing launched: for a
// caller that wants the allocation (which may synchronise the device) ahead
// of the kernel that produces `in`; exclusive_scan then finds tmp large enough.
static inline int scan_reserve(DevBuf &tmp, const int *in, int *out, int n, hipStream_t s, size_t *tb, char *msg,
                               size_t msglen) {
  DEVCK(hipcub::DeviceScan::ExclusiveSum(nullptr, *tb, in, out, n, s));
  if (!get<char>(tmp, *tb)) {
    snprintf(msg, msglen, "out of device memory (scan)");
    return 0;
  }
  return 1;
}

// out[i] = in[0] + ... + in[i - 1], i < n, on stream s
static inline int exclusive_scan(DevBuf &tmp, const int *in, int *out, int n, hipStream_t s, char *msg, size_t msglen) {
  size_t tb = 0;
  if (!scan_reserve(tmp, in, out, n, s, &tb, msg, msglen)) return 0;
  DEVCK(hipcub::DeviceScan::ExclusiveSum(tmp.p, tb, in, out, n, s));
  return 1;
}
