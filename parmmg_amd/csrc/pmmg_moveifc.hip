// pmmg_moveifc.hip — the interface displacement of a partition on the device
// (DESIGN.md §13): what PMMG_mark_interfacePoints and the layer loop of
// PMMG_part_moveInterfaces (reference src/moveinterfaces_pmmg.c:1052-1090,
// :1366-1439, with PMMG_mark_boulevolp and PMMG_mark_sideFront) leave in the
// tetra marks and the point colours, as a function of (tetv, mark, weight)
// instead of a loop over points and a walk around each (the definition is in
// include/parmmg_hip.h, "Interface displacement").
//
// Everything is tetra-centric: no list of the tetra around a point, no walk.
//
// Seed.  Every corner 4 k + c of a used tetra lowers two 64-bit words of its
// point: the corner itself, and (weight of the tetra's mark << 32 | corner)
// (atomic_lower, pmmg_devutil.hpp).  A pass over the points reads
// the colour and the front flag off the two words.
//
// A layer works on copies and is committed as a whole or not at all:
//   k_ifc_sweep    per tetra: its front points in ascending id (a sorting
//                  network in registers), the running strict minimum of weight,
//                  the events; the new mark; per event the previous colour's
//                  count in a CountTable in LDS, flushed once per block and colour;
//                  the points off the front get (weight << 32 | point of the
//                  last event) by atomicMin, the other front points a plain
//                  store of 1 in `side`
//   k_ifc_side     per tetra with a side point: (weight of the new mark << 32
//                  | tetra) by atomicMin into the side points' words
//   k_ifc_points   per point: the new colour and front flag off the two words
// The host reads D and the count of re-marked tetra (one synchronisation per
// layer), decides the brake (pmmg_moveifc_decide.hpp) and swaps the copies.
// The first layer of a call reads the caller's arrays where they are; only
// the last committed state is copied out.
// No kernel waits on another workgroup's store.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdio.h>

#include <vector>

#include "pmmg_devutil.hpp"
#include "pmmg_moveifc.hpp"
#include "pmmg_moveifc_decide.hpp"

namespace {

// the events of a block per previous colour: 1024 slots, 8 tried before a count goes to the colour's word directly
typedef CountTable<1024, 8> EventTable;

typedef unsigned long long u64;
constexpr u64 kNone = ~0ULL;

// the calls' flag bits
enum { I_BADMARK = 1, I_BADVERT = 2, I_BADCOLOR = 4, I_BADSET = 8, I_BADSETCOLOR = 16 };
// the calls' words on the device
enum { W_FLAGS = 0, W_MOVED = 1, W_COUNT = 4 };

struct MMesh : TetRows {
  int np;
};

// The refusals of a mesh with marks: a mark of a used tetra outside [0, ncolor), a vertex id outside [1, np];
// with ptcolor, a point of a used tetra whose colour lies outside [0, ncolor).
__global__ __launch_bounds__(kPBlock) void k_ifc_check(MMesh m, const int *mark, int ncolor, const int *ptcolor,
                                                       int *flags) {
  int bad = 0;
  const int stride = (int)gridDim.x * kPBlock;
  for (int k = (int)blockIdx.x * kPBlock + (int)threadIdx.x; k < m.ne; k += stride) {
    const int4 v = m.tetv[(size_t)k * m.tstride];
    if (v.x <= 0) continue;
    if ((unsigned int)mark[k] >= (unsigned int)ncolor) bad |= I_BADMARK;
    const int vv[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
    for (int c = 0; c < 4; c++) {
      if ((unsigned int)(vv[c] - 1) >= (unsigned int)m.np)
        bad |= I_BADVERT;
      else if (ptcolor && (unsigned int)ptcolor[vv[c] - 1] >= (unsigned int)ncolor)
        bad |= I_BADCOLOR;
    }
  }
  if (bad) atomicOr(flags, bad);
}

__global__ __launch_bounds__(kPBlock) void k_ifc_check_set(int np, int ncolor, int nset, const int *set_pt,
                                                           const int *set_color, int *flags) {
  const int i = (int)blockIdx.x * kPBlock + (int)threadIdx.x;
  if (i >= nset) return;
  int bad = 0;
  if ((unsigned int)(set_pt[i] - 1) >= (unsigned int)np) bad |= I_BADSET;
  if (set_color && (unsigned int)set_color[i] >= (unsigned int)ncolor) bad |= I_BADSETCOLOR;
  if (bad) atomicOr(flags, bad);
}

// ---- the seed

__global__ __launch_bounds__(kPBlock) void k_ifc_seed_min(MMesh m, const int *mark, const int *weight, u64 *first,
                                                          u64 *best) {
  const int stride = (int)gridDim.x * kPBlock;
  for (int k = (int)blockIdx.x * kPBlock + (int)threadIdx.x; k < m.ne; k += stride) {
    const int4 v = m.tetv[(size_t)k * m.tstride];
    if (v.x <= 0) continue;
    const int vv[4] = {v.x, v.y, v.z, v.w};
    const u64 wk = (u64)(unsigned int)weight[mark[k]] << 32;
#pragma unroll
    for (int c = 0; c < 4; c++) {
      const u64 corner = (u64)(unsigned int)(4 * k + c);
      atomic_lower(&first[vv[c] - 1], corner);
      atomic_lower(&best[vv[c] - 1], wk | corner);
    }
  }
}

__global__ __launch_bounds__(kPBlock) void k_ifc_seed_points(int np, const int *mark, const int *weight,
                                                             const u64 *first, const u64 *best, int *ptcolor,
                                                             unsigned char *ptfront) {
  const int stride = (int)gridDim.x * kPBlock;
  for (int p = (int)blockIdx.x * kPBlock + (int)threadIdx.x; p < np; p += stride) {
    const u64 f = first[p], b = best[p];
    if (f == kNone) { // in no used tetra
      ptcolor[p] = -1;
      ptfront[p] = 0;
      continue;
    }
    ptcolor[p] = mark[(unsigned int)(b & 0xffffffffu) >> 2];
    ptfront[p] = (unsigned int)weight[mark[(unsigned int)f >> 2]] != (unsigned int)(b >> 32) ? 1 : 0;
  }
}

// ---- a layer

// The set points of a layer become front (and take their colours); what they held is kept for a layer that is
// dropped.  The entries of set_pt are distinct.
__global__ __launch_bounds__(kPBlock) void k_ifc_set(int nset, const int *set_pt, const int *set_color, int *color,
                                                     unsigned char *front, int *old_color, unsigned char *old_front) {
  const int i = (int)blockIdx.x * kPBlock + (int)threadIdx.x;
  if (i >= nset) return;
  const int p = set_pt[i] - 1;
  old_color[i] = color[p];
  old_front[i] = front[p];
  front[p] = 1;
  if (set_color) color[p] = set_color[i];
}

__global__ __launch_bounds__(kPBlock) void k_ifc_unset(int nset, const int *set_pt, const int *old_color,
                                                       const unsigned char *old_front, int *color,
                                                       unsigned char *front) {
  const int i = (int)blockIdx.x * kPBlock + (int)threadIdx.x;
  if (i >= nset) return;
  const int p = set_pt[i] - 1;
  color[p] = old_color[i];
  front[p] = old_front[i];
}

__device__ __forceinline__ void cswap(int &a, int &b) {
  const int lo = a < b ? a : b, hi = a < b ? b : a;
  a = lo;
  b = hi;
}

__global__ __launch_bounds__(kPBlock) void k_ifc_sweep(MMesh m, const int *mark, const int *weight, const int *color,
                                                       const unsigned char *front, int *nmark, u64 *ekey,
                                                       unsigned char *side, int *D, int *moved) {
  __shared__ EventTable events;
  __shared__ int s_moved;
  const auto count_of = [D](int g) { return &D[g]; };
  events.clear<kPBlock>();
  if (threadIdx.x == 0) s_moved = 0;
  __syncthreads();
  int nmoved = 0;
  const int stride = (int)gridDim.x * kPBlock;
  for (int k = (int)blockIdx.x * kPBlock + (int)threadIdx.x; k < m.ne; k += stride) {
    const int4 v = m.tetv[(size_t)k * m.tstride];
    const int mk = mark[k];
    if (v.x <= 0) {
      nmark[k] = mk;
      continue;
    }
    int a = v.x, b = v.y, c = v.z, d = v.w; // ascending point id
    cswap(a, b);
    cswap(c, d);
    cswap(a, c);
    cswap(b, d);
    cswap(b, c);
    const int id[4] = {a, b, c, d};
    bool fr[4];
#pragma unroll
    for (int j = 0; j < 4; j++) fr[j] = front[id[j] - 1] != 0;
    int cur = mk, curw = weight[mk], nev = 0, last = 0;
#pragma unroll
    for (int j = 0; j < 4; j++) {
      if (!fr[j]) continue;
      const int C = color[id[j] - 1], wc = weight[C];
      if (wc < curw) { // an event: C beats the running colour
        events.add(cur, 1, count_of);
        cur = C;
        curw = wc;
        nev++;
        last = id[j];
      }
    }
    nmark[k] = cur;
    if (!nev) continue;
    nmoved++;
    const u64 key = ((u64)(unsigned int)curw << 32) | (u64)(unsigned int)last;
#pragma unroll
    for (int j = 0; j < 4; j++) {
      if (!fr[j])
        atomic_lower(&ekey[id[j] - 1], key);
      else if (nev > 1 || id[j] != last)
        side[id[j] - 1] = 1;
    }
  }
  if (nmoved) atomicAdd(&s_moved, nmoved);
  __syncthreads();
  events.flush<kPBlock>(count_of);
  if (threadIdx.x == 0 && s_moved) atomicAdd(moved, s_moved);
}

__global__ __launch_bounds__(kPBlock) void k_ifc_side(MMesh m, const int *nmark, const int *weight,
                                                      const unsigned char *side, u64 *skey) {
  const int stride = (int)gridDim.x * kPBlock;
  for (int k = (int)blockIdx.x * kPBlock + (int)threadIdx.x; k < m.ne; k += stride) {
    const int4 v = m.tetv[(size_t)k * m.tstride];
    if (v.x <= 0) continue;
    const int vv[4] = {v.x, v.y, v.z, v.w};
    bool sd[4];
#pragma unroll
    for (int c = 0; c < 4; c++) sd[c] = side[vv[c] - 1] != 0;
    if (!(sd[0] | sd[1] | sd[2] | sd[3])) continue;
    const u64 key = ((u64)(unsigned int)weight[nmark[k]] << 32) | (u64)(unsigned int)k;
#pragma unroll
    for (int c = 0; c < 4; c++)
      if (sd[c]) atomic_lower(&skey[vv[c] - 1], key);
  }
}

__global__ __launch_bounds__(kPBlock) void k_ifc_points(int np, const int *nmark, const int *weight, const int *color,
                                                        const u64 *ekey, const u64 *skey, const unsigned char *side,
                                                        int *ncolor_out, unsigned char *nfront) {
  const int stride = (int)gridDim.x * kPBlock;
  for (int p = (int)blockIdx.x * kPBlock + (int)threadIdx.x; p < np; p += stride) {
    const int c = color[p];
    const u64 e = ekey[p];
    const bool sd = side[p] != 0;
    int out = c;
    if (e != kNone || sd) { // (a point of a used tetra: its colour is a colour)
      const unsigned int wq = (unsigned int)weight[c];
      if (e != kNone && (unsigned int)(e >> 32) < wq) out = color[(unsigned int)(e & 0xffffffffu) - 1];
      if (sd) {
        const u64 sk = skey[p];
        if ((unsigned int)(sk >> 32) < wq) out = nmark[(unsigned int)(sk & 0xffffffffu)];
      }
    }
    ncolor_out[p] = out;
    nfront[p] = (e != kNone || sd) ? 1 : 0;
  }
}

// ---- the packing of the colours

__global__ __launch_bounds__(kPBlock) void k_ifc_present(MMesh m, const int *mark, int ncolor, unsigned char *present,
                                                         int *flags) {
  bool bad = false;
  const int stride = (int)gridDim.x * kPBlock;
  for (int k = (int)blockIdx.x * kPBlock + (int)threadIdx.x; k < m.ne; k += stride) {
    if (m.tetv[(size_t)k * m.tstride].x <= 0) continue;
    const int g = mark[k];
    if ((unsigned int)g >= (unsigned int)ncolor)
      bad = true;
    else if (!present[g]) // (plain stores of the same value)
      present[g] = 1;
  }
  if (bad) atomicOr(flags, (int)I_BADMARK);
}

__global__ __launch_bounds__(kPBlock) void k_ifc_apply(MMesh m, const int *mark, const int *map, int *part) {
  const int stride = (int)gridDim.x * kPBlock;
  for (int k = (int)blockIdx.x * kPBlock + (int)threadIdx.x; k < m.ne; k += stride)
    part[k] = m.tetv[(size_t)k * m.tstride].x <= 0 ? 0 : map[mark[k]];
}

int bad_weight(int ncolor, const int *weight, const char *who, char *msg, size_t msglen) {
  for (int c = 0; c < ncolor; c++)
    if (weight[c] <= 0) {
      snprintf(msg, msglen, "%s: weight[%d] = %d is not positive (nothing written)", who, c, weight[c]);
      return 1;
    }
  return 0;
}

int refused(int f, const char *who, int ncolor, int np, char *msg, size_t msglen) {
  if (f & I_BADMARK)
    snprintf(msg, msglen, "%s: a mark lies outside [0, %d) (nothing written)", who, ncolor);
  else if (f & I_BADVERT)
    snprintf(msg, msglen, "%s: a vertex id lies outside [1, %d] (nothing written)", who, np);
  else if (f & I_BADCOLOR)
    snprintf(msg, msglen, "%s: the colour of a point of a used tetra lies outside [0, %d) (nothing written)", who,
             ncolor);
  else if (f & I_BADSET)
    snprintf(msg, msglen, "%s: a set_pt entry lies outside [1, %d] (nothing written)", who, np);
  else if (f & I_BADSETCOLOR)
    snprintf(msg, msglen, "%s: a set_color entry lies outside [0, %d) (nothing written)", who, ncolor);
  return f != 0;
}

} // namespace

int pmmg_ifc_seed(hipStream_t s, int np, TetView tv, const int *mark, int ncolor, const int *weight, int *ptcolor,
                  unsigned char *ptfront, MoveCache *c, char *msg, size_t msglen) {
  if (bad_weight(ncolor, weight, "ifc_seed", msg, msglen)) return 0;
  const int ne = tv.ne;
  int *words = get<int>(c->words, W_COUNT), *wdev = get<int>(c->weight, (size_t)ncolor);
  u64 *first = get<u64>(c->key[0], (size_t)np), *best = get<u64>(c->key[1], (size_t)np);
  if (!words || !wdev || !first || !best) {
    snprintf(msg, msglen, "ifc_seed: out of device memory (scratch of %d points, %d colours)", np, ncolor);
    return 0;
  }
  const MMesh m{rows_of(tv), np};
  DEVCK(hipMemsetAsync(words, 0, W_COUNT * sizeof(int), s));
  if (ne > 0) {
    hipLaunchKernelGGL(k_ifc_check, dim3(grid_for(ne)), dim3(kPBlock), 0, s, m, mark, ncolor, (const int *)nullptr,
                       words + W_FLAGS);
    DEVCK(hipGetLastError());
  }
  int f = 0;
  if (!read_word(s, words + W_FLAGS, &f, msg, msglen)) return 0;
  if (refused(f, "ifc_seed", ncolor, np, msg, msglen)) return 0;
  if (np == 0) return 1;
  DEVCK(hipMemcpyAsync(wdev, weight, sizeof(int) * (size_t)ncolor, hipMemcpyHostToDevice, s));
  DEVCK(hipMemsetAsync(first, 0xff, sizeof(u64) * (size_t)np, s));
  DEVCK(hipMemsetAsync(best, 0xff, sizeof(u64) * (size_t)np, s));
  if (ne > 0) hipLaunchKernelGGL(k_ifc_seed_min, dim3(grid_for(ne)), dim3(kPBlock), 0, s, m, mark, wdev, first, best);
  hipLaunchKernelGGL(k_ifc_seed_points, dim3(grid_for(np)), dim3(kPBlock), 0, s, np, mark, wdev, first, best, ptcolor,
                     ptfront);
  DEVCK(hipGetLastError());
  DEVCK(hipStreamSynchronize(s)); // (the copy of `weight`, a pageable host array, is done too)
  return 1;
}

int pmmg_ifc_layers(hipStream_t s, int np, TetView tv, int *mark, int ncolor, const int *weight, int *nelem,
                    const int *nemin, int *ptcolor, unsigned char *ptfront, int nset, const int *set_pt,
                    const int *set_color, int nlayers, int *layers_done, int *blocked, int *moved, MoveCache *c,
                    char *msg, size_t msglen) {
  if (bad_weight(ncolor, weight, "ifc_layers", msg, msglen)) return 0;
  const int ne = tv.ne;
  int *words = get<int>(c->words, W_COUNT), *wdev = get<int>(c->weight, (size_t)ncolor);
  int *D = get<int>(c->D, (size_t)ncolor);
  u64 *ekey = get<u64>(c->key[0], (size_t)np), *skey = get<u64>(c->key[1], (size_t)np);
  unsigned char *side = get<unsigned char>(c->side, (size_t)np);
  int *mk[2] = {get<int>(c->mark[0], (size_t)ne), get<int>(c->mark[1], (size_t)ne)};
  int *col[2] = {get<int>(c->color[0], (size_t)np), get<int>(c->color[1], (size_t)np)};
  unsigned char *fr[2] = {get<unsigned char>(c->front[0], (size_t)np), get<unsigned char>(c->front[1], (size_t)np)};
  int *old_color = get<int>(c->set_color, (size_t)nset);
  unsigned char *old_front = get<unsigned char>(c->set_front, (size_t)nset);
  if (!words || !wdev || !D || !ekey || !skey || !side || !mk[0] || !mk[1] || !col[0] || !col[1] || !fr[0] || !fr[1] ||
      !old_color || !old_front) {
    snprintf(msg, msglen, "ifc_layers: out of device memory (scratch of %d tetra, %d points, %d colours)", ne, np,
             ncolor);
    return 0;
  }
  const MMesh m{rows_of(tv), np};
  const int grid = grid_for(ne), pgrid = grid_for(np), sgrid = (nset + kPBlock - 1) / kPBlock;

  // the refusals: nothing is written to an output before they are known
  DEVCK(hipMemsetAsync(words, 0, W_COUNT * sizeof(int), s));
  if (ne > 0) hipLaunchKernelGGL(k_ifc_check, dim3(grid), dim3(kPBlock), 0, s, m, mark, ncolor, ptcolor, words + W_FLAGS);
  if (nset > 0)
    hipLaunchKernelGGL(k_ifc_check_set, dim3(sgrid), dim3(kPBlock), 0, s, np, ncolor, nset, set_pt, set_color,
                       words + W_FLAGS);
  DEVCK(hipGetLastError());
  int f = 0;
  if (!read_word(s, words + W_FLAGS, &f, msg, msglen)) return 0;
  if (refused(f, "ifc_layers", ncolor, np, msg, msglen)) return 0;
  *layers_done = 0;
  *blocked = 0;
  for (int l = 0; l < nlayers; l++) moved[l] = 0;
  if (ne == 0 || np == 0 || nlayers == 0) return 1;

  DEVCK(hipMemcpyAsync(wdev, weight, sizeof(int) * (size_t)ncolor, hipMemcpyHostToDevice, s));
  // The first layer reads the caller's arrays where they are; every layer writes into the scratch, and only the
  // last committed state is copied out.  Set points are written into the state a layer reads: with them the point
  // state is copied in first.
  const int *cm = mark, *cc = ptcolor;
  const unsigned char *cf = ptfront;
  int wm = 0, wp = 0; // the scratch copies the next layer writes
  if (nset > 0) {
    DEVCK(hipMemcpyAsync(col[0], ptcolor, sizeof(int) * (size_t)np, hipMemcpyDeviceToDevice, s));
    DEVCK(hipMemcpyAsync(fr[0], ptfront, (size_t)np, hipMemcpyDeviceToDevice, s));
    cc = col[0];
    cf = fr[0];
    wp = 1;
  }
  std::vector<int> hD((size_t)ncolor);
  for (int l = 0; l < nlayers; l++) {
    int *nm = mk[wm], *nc = col[wp];
    unsigned char *nf = fr[wp];
    if (nset > 0) // (cc / cf are scratch copies here)
      hipLaunchKernelGGL(k_ifc_set, dim3(sgrid), dim3(kPBlock), 0, s, nset, set_pt, l == 0 ? set_color : nullptr,
                         const_cast<int *>(cc), const_cast<unsigned char *>(cf), old_color, old_front);
    DEVCK(hipMemsetAsync(ekey, 0xff, sizeof(u64) * (size_t)np, s));
    DEVCK(hipMemsetAsync(skey, 0xff, sizeof(u64) * (size_t)np, s));
    DEVCK(hipMemsetAsync(side, 0, (size_t)np, s));
    DEVCK(hipMemsetAsync(D, 0, sizeof(int) * (size_t)ncolor, s));
    DEVCK(hipMemsetAsync(words + W_MOVED, 0, sizeof(int), s));
    hipLaunchKernelGGL(k_ifc_sweep, dim3(grid), dim3(kPBlock), 0, s, m, cm, wdev, cc, cf, nm, ekey, side, D,
                       words + W_MOVED);
    hipLaunchKernelGGL(k_ifc_side, dim3(grid), dim3(kPBlock), 0, s, m, nm, wdev, side, skey);
    hipLaunchKernelGGL(k_ifc_points, dim3(pgrid), dim3(kPBlock), 0, s, np, nm, wdev, cc, ekey, skey, side, nc, nf);
    DEVCK(hipGetLastError());
    int nmoved = 0;
    DEVCK(hipMemcpyAsync(hD.data(), D, sizeof(int) * (size_t)ncolor, hipMemcpyDeviceToHost, s));
    if (!read_word(s, words + W_MOVED, &nmoved, msg, msglen)) return 0;
    if (ifc_first_braked(ncolor, hD.data(), nelem, nemin) >= 0) {
      // the layer is dropped, its set points with it: the outputs are the previous layer's
      *blocked = 1;
      if (nset > 0 && l > 0)
        hipLaunchKernelGGL(k_ifc_unset, dim3(sgrid), dim3(kPBlock), 0, s, nset, set_pt, old_color, old_front,
                           const_cast<int *>(cc), const_cast<unsigned char *>(cf));
      DEVCK(hipGetLastError());
      break;
    }
    ifc_commit_counts(ncolor, hD.data(), nelem);
    moved[l] = nmoved;
    *layers_done = l + 1;
    cm = nm;
    cc = nc;
    cf = nf;
    wm ^= 1;
    wp ^= 1;
  }
  if (*layers_done > 0) {
    DEVCK(hipMemcpyAsync(mark, cm, sizeof(int) * (size_t)ne, hipMemcpyDeviceToDevice, s));
    DEVCK(hipMemcpyAsync(ptcolor, cc, sizeof(int) * (size_t)np, hipMemcpyDeviceToDevice, s));
    DEVCK(hipMemcpyAsync(ptfront, cf, (size_t)np, hipMemcpyDeviceToDevice, s));
  }
  DEVCK(hipStreamSynchronize(s));
  return 1;
}

int pmmg_ifc_remap(hipStream_t s, TetView tv, const int *mark, int ncolor, const int *order, int *part, int *ngrp,
                   MoveCache *c, char *msg, size_t msglen) {
  const int ne = tv.ne;
  // present[ncolor] bytes rounded up to whole ints, then map[ncolor]
  const size_t pwords = ((size_t)ncolor + 3) / 4;
  int *words = get<int>(c->words, W_COUNT), *buf = get<int>(c->map, pwords + (size_t)ncolor);
  if (!words || !buf) {
    snprintf(msg, msglen, "remap_colors: out of device memory (%d colours)", ncolor);
    return 0;
  }
  if (ne == 0) {
    *ngrp = 0;
    return 1;
  }
  unsigned char *present = reinterpret_cast<unsigned char *>(buf);
  int *map = buf + pwords;
  const MMesh m{rows_of(tv), 0};
  DEVCK(hipMemsetAsync(words, 0, W_COUNT * sizeof(int), s));
  DEVCK(hipMemsetAsync(present, 0, pwords * sizeof(int), s));
  hipLaunchKernelGGL(k_ifc_present, dim3(grid_for(ne)), dim3(kPBlock), 0, s, m, mark, ncolor, present, words + W_FLAGS);
  DEVCK(hipGetLastError());
  std::vector<unsigned char> hp((size_t)ncolor);
  std::vector<int> hmap((size_t)ncolor);
  DEVCK(hipMemcpyAsync(hp.data(), present, (size_t)ncolor, hipMemcpyDeviceToHost, s));
  int f = 0;
  if (!read_word(s, words + W_FLAGS, &f, msg, msglen)) return 0;
  if (refused(f, "remap_colors", ncolor, 0, msg, msglen)) return 0;
  *ngrp = ifc_pack_colors(ncolor, hp.data(), order, hmap.data());
  DEVCK(hipMemcpyAsync(map, hmap.data(), sizeof(int) * (size_t)ncolor, hipMemcpyHostToDevice, s));
  hipLaunchKernelGGL(k_ifc_apply, dim3(grid_for(ne)), dim3(kPBlock), 0, s, m, mark, map, part);
  DEVCK(hipGetLastError());
  DEVCK(hipStreamSynchronize(s));
  return 1;
}
