// pmmg_blockscan.hpp — the prefix and the reduction of one int per thread over a block, for every kernel of
// the library (the transfer call's through pmmg_prep.hpp, the mesh services' through pmmg_devutil.hpp).
// Nothing but HIP itself is included here.
#pragma once
#include <hip/hip_runtime.h>

// The sum of c over the threads before this one and, in every thread, the block's sum in *total.  All
// 64 * WAVES threads of the block call it; wt has WAVES ints.  No barrier after wt is read: a caller
// that uses wt again synchronises first.  The sums are plain int additions, so a value that packs two
// counters whose block sums stay in their fields ({flag << 16 | count}) is prefixed field by field.
template <int WAVES>
__device__ __forceinline__ int block_prefix(int c, int *wt, int *total) {
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  int x = c; // inclusive prefix within the wave
  for (int o = 1; o < 64; o <<= 1) {
    const int y = __shfl_up(x, o);
    if (lane >= o) x += y;
  }
  if (lane == 63) wt[w] = x;
  __syncthreads();
  int pos = x - c, t = 0;
  for (int i = 0; i < WAVES; i++) {
    if (i < w) pos += wt[i];
    t += wt[i];
  }
  *total = t;
  return pos;
}

struct IntSum { __device__ int operator()(int a, int b) const { return a + b; } };
struct IntMax { __device__ int operator()(int a, int b) const { return a > b ? a : b; } };

// op over the block's values of c, in thread 0 (the other threads get a partial).  Same contract as
// block_prefix: all 64 * WAVES threads, wt of WAVES ints, no barrier at the end.
template <int WAVES, class Op>
__device__ __forceinline__ int block_reduce(int c, int *wt, Op op) {
  for (int o = 32; o > 0; o >>= 1) c = op(c, __shfl_down(c, o));
  if ((threadIdx.x & 63) == 0) wt[threadIdx.x >> 6] = c;
  __syncthreads();
  if (threadIdx.x == 0)
    for (int w = 1; w < WAVES; w++) c = op(c, wt[w]);
  return c;
}
