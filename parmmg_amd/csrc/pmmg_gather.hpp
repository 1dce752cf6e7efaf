// pmmg_gather.hpp — internal interface of pmmg_gather.hip (the rows of an array through a map: what a caller
// of the split and the merge does with old_pt, src_pt and src_tet); the C-ABI wrappers live in pmmg_hip.hip.
#pragma once
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

// out row r = in row src[r] - 1, r < n.  A row is row_bytes bytes, a whole number of elements of elem_bytes
// (4 or 8) bytes, and in and out are aligned to an element.  Asynchronous on s.  Returns 1, or 0 with msg set.
int pmmg_gather_rows(hipStream_t s, int64_t n, const int *src, int64_t row_bytes, int elem_bytes, const void *in,
                     void *out, char *msg, size_t msglen);
