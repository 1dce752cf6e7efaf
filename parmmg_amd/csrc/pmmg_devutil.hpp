// pmmg_devutil.hpp — what the mesh services (pmmg_snapshot.hip, pmmg_meshstats.hip, pmmg_graph.hip,
// pmmg_contig.hip, pmmg_split.hip, pmmg_moveifc.hip, pmmg_merge.hip, pmmg_gather.hip) share.  Device side
// (beside pmmg_blockscan.hpp's prefix and reduction over a block): the block and grid of the group services,
// the tetra rows as a kernel reads them, the range check of a link, the flag bits of a pass over the links,
// the kernel that looks for a link to an unused row, the guarded atomic minimum, the count table of a block
// in LDS.  Host side: the error macro of a function that reports through (msg, msglen) and returns 0, a word
// read back, the exclusive scan of an int array, the two operations of a BlockScan, and the two steps the
// graph and the contiguity calls share.
#pragma once
#include <hip/hip_runtime.h>
#include <hipcub/hipcub.hpp>

#include <stdio.h>

#include "pmmg_blockscan.hpp"
#include "pmmg_devbuf.hpp"
#include "pmmg_snapshot.hpp"

// ---------------------------------------------------------------- device side

// The block of the kernels that serve a partition (kP: contiguity, split, interface displacement, merge,
// gather) and the grid of a grid-stride kernel over n items: an index below 2^29 plus the stride, at most
// 2048 * 256 = 2^19, stays below 2^30, so the loops count in an int.
constexpr int kPBlock = 256;
constexpr int kPWaves = kPBlock / 64;
constexpr int kPMaxBlocks = 2048;

static inline int grid_for(long long n) {
  const long long b = (n + kPBlock - 1) / kPBlock;
  return b < 1 ? 1 : (b > kPMaxBlocks ? kPMaxBlocks : (int)b);
}

// The rows of a TetView as a kernel reads them: one 16-byte load a row.
struct TetRows {
  int ne;
  const int4 *tetv;
  int tstride;
  const int4 *adja;
  int astride;
};
static inline TetRows rows_of(const TetView &v) {
  return TetRows{v.ne, reinterpret_cast<const int4 *>(v.tetv), v.tstride, reinterpret_cast<const int4 *>(v.adja),
                 v.astride};
}

// a link 4 k' + i' of a mesh of ne tetra lies in [4, 4 ne + 3]
__device__ __forceinline__ bool link_ok(int a, int ne) { return (unsigned int)(a - 4) <= 4u * (unsigned int)ne - 1u; }

// *p = min(*p, key): agent scope, relaxed, nothing returned, and no atomic at all when a plain load already
// shows a value that is not above key (words that many threads lower settle early, and most callers then
// only read).  What the word holds afterwards does not depend on the interleaving.
template <class T>
__device__ __forceinline__ void atomic_lower(T *p, T key) {
  if (key < __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT))
    (void)__hip_atomic_fetch_min(p, key, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// The counts of a block per key (a key >= 0: a table row, a colour), in LDS: a __shared__ object, cleared by the
// whole block (BLOCK threads) with a barrier after it, added to by any thread, and flushed by the whole block
// after a barrier, one atomicAdd per key the block met.  word(key) is the key's count in global memory: a key
// that finds PROBE slots taken by others adds there directly.
template <int SLOTS, int PROBE>
struct CountTable {
  static_assert(SLOTS == 1 << 10, "the hash keeps 10 bits");
  int key[SLOTS], cnt[SLOTS];

  template <int BLOCK>
  __device__ __forceinline__ void clear() {
    for (int i = (int)threadIdx.x; i < SLOTS; i += BLOCK) {
      key[i] = -1;
      cnt[i] = 0;
    }
  }
  template <class Word>
  __device__ __forceinline__ void add(int k, int n, Word word) {
    unsigned int h = ((unsigned int)k * 2654435761u) >> 22;
    for (int i = 0; i < PROBE; i++) {
      const int old = atomicCAS(&key[h], -1, k);
      if (old == -1 || old == k) {
        atomicAdd(&cnt[h], n);
        return;
      }
      h = (h + 1) & (SLOTS - 1);
    }
    atomicAdd(word(k), n);
  }
  template <int BLOCK, class Word>
  __device__ __forceinline__ void flush(Word word) {
    for (int i = (int)threadIdx.x; i < SLOTS; i += BLOCK)
      if (key[i] >= 0) atomicAdd(word(key[i]), cnt[i]);
  }
};

// Flag bits of a pass over the links of a mesh.  Bit 2 is the pass's own (a vertex id, a colour).
enum { MESH_BADLINK = 1, MESH_UNUSED = 4, MESH_TOUNUSED = 8 };

// A mesh with unused rows (v[0] <= 0): a link of a used row that points to an unused one (the reference
// requires a packed mesh).  Precondition: every non-zero link is in range (the pass that saw the unused
// rows found no MESH_BADLINK).  Grid-stride: any grid is correct, and k + stride stays an int for ne < 2^29
// and at most ceil(ne / BLOCK) blocks.  (A template, as check_links is: only a file that calls it has the kernel.)
template <int BLOCK>
__global__ __launch_bounds__(BLOCK) void k_links_to_unused(int ne, const int4 *tetv, int tstride, const int4 *adja,
                                                           int astride, int *flags) {
  bool bad = false;
  const int stride = (int)gridDim.x * BLOCK;
  for (int k = (int)blockIdx.x * BLOCK + (int)threadIdx.x; k < ne; k += stride) {
    if (tetv[(size_t)k * tstride].x <= 0) continue;
    const int4 a = adja[(size_t)k * astride];
    const int lk[4] = {a.x, a.y, a.z, a.w};
#pragma unroll
    for (int f = 0; f < 4; f++)
      if (lk[f] && tetv[(size_t)(lk[f] / 4 - 1) * tstride].x <= 0) bad = true;
  }
  if (bad) atomicOr(flags, (int)MESH_TOUNUSED);
}

// ---------------------------------------------------------------- host side

#define DEVCK(expr)                                                                                 \
  do {                                                                                              \
    hipError_t e_ = (expr);                                                                         \
    if (e_ != hipSuccess) {                                                                         \
      snprintf(msg, msglen, "%s failed: %s (%s:%d)", #expr, hipGetErrorString(e_), __FILE__, __LINE__); \
      return 0;                                                                                     \
    }                                                                                               \
  } while (0)

// 0, with `text` in msg
static inline int refuse(char *msg, size_t msglen, const char *text) {
  snprintf(msg, msglen, "%s", text);
  return 0;
}

// a word of the device back on the host; the stream is synchronised
static inline int read_word(hipStream_t s, const int *d, int *h, char *msg, size_t msglen) {
  DEVCK(hipMemcpyAsync(h, d, sizeof(int), hipMemcpyDeviceToHost, s));
  DEVCK(hipStreamSynchronize(s));
  return 1;
}

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

// A BlockScan (pmmg_devbuf.hpp) ahead of its counting kernel: nblk + 1 entries of btot and boff and the
// scan's temporary (an allocation may synchronise the device).  oom: the caller's message when the device
// has no memory for the arrays.
static inline int reserve(BlockScan &b, int nblk, hipStream_t s, const char *oom, char *msg, size_t msglen) {
  const int *in = get<int>(b.btot, (size_t)nblk + 1);
  int *out = get<int>(b.boff, (size_t)nblk + 1);
  if (!in || !out) return refuse(msg, msglen, oom);
  size_t tb = 0;
  return scan_reserve(b.tmp, in, out, nblk + 1, s, &tb, msg, msglen);
}

// after the counting kernel: boff[b] = btot[0] + ... + btot[b - 1], b <= nblk, and with `total` the sum
// boff[nblk] back on the host and the stream synchronised
static inline int offsets(BlockScan &b, hipStream_t s, int nblk, int *total, char *msg, size_t msglen) {
  int *in = b.btot.as<int>(), *out = b.boff.as<int>();
  DEVCK(hipMemsetAsync(in + nblk, 0, sizeof(int), s));
  if (!exclusive_scan(b.tmp, in, out, nblk + 1, s, msg, msglen)) return 0;
  return total ? read_word(s, out + nblk, total, msg, msglen) : 1;
}

// The refusal of a mesh whose pass over the links left MESH_UNUSED in *h_flags (a copy of the device word
// `flags`, no MESH_BADLINK in it): a link to an unused row.  *h_flags is read again after the kernel.
// The message is "<who>: an adja entry points to an unused tetra<tail>".
template <int BLOCK>
int check_links(hipStream_t s, const char *who, const char *tail, const TetView &m, int *flags, int *h_flags,
                char *msg, size_t msglen) {
  if (!(*h_flags & MESH_UNUSED)) return 1;
  const int nblk = (m.ne + BLOCK - 1) / BLOCK;
  const TetRows r = rows_of(m);
  hipLaunchKernelGGL(k_links_to_unused<BLOCK>, dim3(nblk < kPMaxBlocks ? nblk : kPMaxBlocks), dim3(BLOCK), 0, s,
                     m.ne, r.tetv, r.tstride, r.adja, r.astride, flags);
  DEVCK(hipGetLastError());
  if (!read_word(s, flags, h_flags, msg, msglen)) return 0;
  if (*h_flags & MESH_TOUNUSED) {
    snprintf(msg, msglen, "%s: an adja entry points to an unused tetra%s", who, tail);
    return 0;
  }
  return 1;
}

// The link rows of a call that came without any (m->adja NULL, m->tetv unpacked rows with ids in
// [1, np]): built into `store` by pmmg_snap_adjacency, which sets msg when it refuses the mesh.
static inline int built_adjacency(hipStream_t s, const char *who, int np, TetView *m, DevBuf &store, SnapCache *snap,
                                  char *msg, size_t msglen) {
  int *built = get<int>(store, 4 * (size_t)m->ne);
  if (!built) {
    snprintf(msg, msglen, "%s: out of device memory (adjacency of %d tetra)", who, m->ne);
    return 0;
  }
  if (!pmmg_snap_adjacency(s, np, m->ne, m->tetv, built, nullptr, snap, msg, msglen)) return 0;
  m->adja = built;
  m->astride = 1;
  return 1;
}
