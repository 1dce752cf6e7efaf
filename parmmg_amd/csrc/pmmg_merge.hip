// pmmg_merge.hip — the groups of a rank joined into one mesh, on the device
// (DESIGN.md §14): what PMMG_merge_grps steps 0-4 (reference
// src/mergemesh_pmmg.c:1004-1043) leave in group 0 and in the two intvalues
// arrays, as a function of the concatenated groups instead of a sequential
// loop.  The inverse of pmmg_split.hip.
//
// Entries.  The groups arrive concatenated in group order, so an entry's index
// e in the concatenated node (or face) list ascends with (group, entry):
// "first in the reference's loop" is a minimum over e, and every id the loop
// hands out is a prefix sum over e, over the concatenated points or over the
// concatenated tetra.  The group of an index comes from a binary search over
// the ngrp + 1 offsets of its table (built on the host, pmmg_merge_tables.hpp).
//
// Lowest entries.  Launch 1: every node entry of a group >= 1 lowers its
// point's word, every node entry of group 0 its position's word, every face
// entry its position's word and (groups >= 1) its tetra's word, and adds one
// to its face position's count.  Launch 2: the node entries that are their
// point's first lower their position's word and add one to its holder count.
// The atomics are agent scope, relaxed, without return, the minima guarded
// (atomic_lower, pmmg_devutil.hpp); a word sees at most the groups that meet
// at its node or face.  No atomic
// touches a per-group or per-call word, and no kernel waits on another
// workgroup's store.
//
// Counts.  Four flags — a node entry that creates a point, a point no entry
// names, a face entry that is its tetra's first, a tetra no entry names — over
// four index ranges laid end to end in blocks of 256: block totals, one scan,
// block prefixes.  Two emit kernels write the maps, the tetra and the values.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdio.h>

#include <vector>

#include "pmmg_devutil.hpp"
#include "pmmg_merge.hpp"
#include "pmmg_merge_tables.hpp"
#include "pmmg_tetview.hpp"

namespace {

typedef unsigned int u32;
constexpr u32 kNoEntry = ~0u;

// the check's flag bits
enum { G_BADVERT = 1, G_BADNODE1 = 2, G_BADNODE2 = 4, G_BADFACE1 = 8, G_BADFACE2 = 16 };
// the four flags, in the order of their ranges in the count and prefix kernels
enum { D_CRE = 0, D_UNL = 1, D_FT = 2, D_INT = 3, D_KINDS = 4 };

// what the passes read and the scratch they share
struct MView {
  int ngrp;
  int T, P, Ef, En; // concatenated tetra, points, face entries, node entries
  int nnode, nface; // positions
  const int *te_off, *pt_off, *fa_off, *no_off, *color;
  const int4 *tetv;
  int tstride;
  const int *n1, *n2, *f1, *f2;
  u32 *ptfirst, *tetfirst, *posmin, *fmin; // lowest entries: [P], [T], [nnode], [nface]
  int *hold, *fcnt;                        // [nnode], [nface]
  int *pre_cre, *pre_unl, *pre_ft, *pre_int; // [En + 1], [P + 1], [Ef + 1], [T + 1]
  int b1, b2, b3;                            // the first block of the ranges D_UNL, D_FT, D_INT
};

struct MOut {
  int *new_pt, *new_tet, *src_pt, *src_tet;
  int4 *tetv_out;
  int *mark_out, *node_val, *face_val;
};

__device__ __forceinline__ void add32(int *p) {
  (void)__hip_atomic_fetch_add(p, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// the group g < ngrp with off[g] <= i < off[g + 1] (i below off[ngrp]; empty groups are passed over)
__device__ __forceinline__ int group_of(const int *off, int ngrp, int i) {
  int lo = 0, hi = ngrp;
  while (hi - lo > 1) {
    const int mid = (lo + hi) >> 1;
    if (off[mid] <= i) lo = mid;
    else hi = mid;
  }
  return lo;
}

// The refusals.  Nothing is written but the flag word.
__global__ __launch_bounds__(kPBlock) void k_merge_check(MView m, int n, int *flags) {
  int bad = 0;
  const int stride = (int)gridDim.x * kPBlock;
  for (int i = (int)blockIdx.x * kPBlock + (int)threadIdx.x; i < n; i += stride) {
    if (i < m.T) {
      const int g = group_of(m.te_off, m.ngrp, i);
      const u32 npg = (u32)(m.pt_off[g + 1] - m.pt_off[g]);
      const int4 v = m.tetv[(size_t)i * m.tstride];
      if ((u32)(v.x - 1) >= npg || (u32)(v.y - 1) >= npg || (u32)(v.z - 1) >= npg || (u32)(v.w - 1) >= npg)
        bad |= G_BADVERT;
    }
    if (i < m.En) {
      const int g = group_of(m.no_off, m.ngrp, i);
      if ((u32)(m.n1[i] - 1) >= (u32)(m.pt_off[g + 1] - m.pt_off[g])) bad |= G_BADNODE1;
      if ((u32)m.n2[i] >= (u32)m.nnode) bad |= G_BADNODE2;
    }
    if (i < m.Ef) {
      const int g = group_of(m.fa_off, m.ngrp, i);
      if ((u32)(m.f1[i] / 12 - 1) >= (u32)(m.te_off[g + 1] - m.te_off[g])) bad |= G_BADFACE1;
      if ((u32)m.f2[i] >= (u32)m.nface) bad |= G_BADFACE2;
    }
  }
  if (bad) atomicOr(flags, bad);
}

// Launch 1 of the lowest entries (the header of this file).
__global__ __launch_bounds__(kPBlock) void k_merge_first(MView m, int n) {
  const int stride = (int)gridDim.x * kPBlock;
  for (int e = (int)blockIdx.x * kPBlock + (int)threadIdx.x; e < n; e += stride) {
    if (e < m.En) {
      if (e < m.no_off[1]) {
        atomic_lower(&m.posmin[m.n2[e]], (u32)e);
      } else {
        const int g = group_of(m.no_off, m.ngrp, e);
        atomic_lower(&m.ptfirst[m.pt_off[g] + m.n1[e] - 1], (u32)e);
      }
    }
    if (e < m.Ef) {
      const int q = m.f2[e];
      atomic_lower(&m.fmin[q], (u32)e);
      if (e >= m.fa_off[1]) {
        const int g = group_of(m.fa_off, m.ngrp, e);
        atomic_lower(&m.tetfirst[m.te_off[g] + m.f1[e] / 12 - 1], (u32)e);
        add32(&m.fcnt[q]);
      }
    }
  }
}

// Launch 2: a point's first entry holds its position.
__global__ __launch_bounds__(kPBlock) void k_merge_pos(MView m) {
  const int stride = (int)gridDim.x * kPBlock;
  for (int e = m.no_off[1] + (int)blockIdx.x * kPBlock + (int)threadIdx.x; e < m.En; e += stride) {
    const int g = group_of(m.no_off, m.ngrp, e);
    if (m.ptfirst[m.pt_off[g] + m.n1[e] - 1] != (u32)e) continue;
    const int p = m.n2[e];
    atomic_lower(&m.posmin[p], (u32)e);
    add32(&m.hold[p]);
  }
}

// the range of a block of the count and prefix kernels, its length, and its prefix array
__device__ __forceinline__ int range_of(const MView &m, int b) { return (b >= m.b1) + (b >= m.b2) + (b >= m.b3); }
__device__ __forceinline__ int range_first(const MView &m, int d) {
  return d == D_CRE ? 0 : (d == D_UNL ? m.b1 : (d == D_FT ? m.b2 : m.b3));
}
__device__ __forceinline__ int range_len(const MView &m, int d) {
  return d == D_CRE ? m.En : (d == D_UNL ? m.P : (d == D_FT ? m.Ef : m.T));
}
__device__ __forceinline__ int *range_pre(const MView &m, int d) {
  return d == D_CRE ? m.pre_cre : (d == D_UNL ? m.pre_unl : (d == D_FT ? m.pre_ft : m.pre_int));
}

// the flag of index i of range d (0 from the range's length on: every range has one more item than entries)
__device__ __forceinline__ int flag_of(const MView &m, int d, int i) {
  if (d == D_CRE) { // a node entry of a group >= 1, its point's first and its position's lowest: a new point
    if (i >= m.En || i < m.no_off[1]) return 0;
    const int g = group_of(m.no_off, m.ngrp, i);
    return m.ptfirst[m.pt_off[g] + m.n1[i] - 1] == (u32)i && m.posmin[m.n2[i]] == (u32)i;
  }
  if (d == D_UNL) return i < m.P && i >= m.pt_off[1] && m.ptfirst[i] == kNoEntry;
  if (d == D_FT) {
    if (i >= m.Ef || i < m.fa_off[1]) return 0;
    const int g = group_of(m.fa_off, m.ngrp, i);
    return m.tetfirst[m.te_off[g] + m.f1[i] / 12 - 1] == (u32)i;
  }
  return i < m.T && i >= m.te_off[1] && m.tetfirst[i] == kNoEntry;
}

// btot[b] = the flags of block b
__global__ __launch_bounds__(kPBlock) void k_merge_counts(MView m, int *btot) {
  __shared__ int wt[kPWaves];
  const int b = (int)blockIdx.x, d = range_of(m, b);
  const int i = (b - range_first(m, d)) * kPBlock + (int)threadIdx.x;
  const int t = block_reduce<kPWaves>(flag_of(m, d, i), wt, IntSum());
  if (threadIdx.x == 0) btot[b] = t;
}

// pre[i] = the flags of the range before i; pre[length] = all of them
__global__ __launch_bounds__(kPBlock) void k_merge_prefix(MView m, const int *boff) {
  __shared__ int wt[kPWaves];
  const int b = (int)blockIdx.x, d = range_of(m, b), b0 = range_first(m, d);
  const int i = (b - b0) * kPBlock + (int)threadIdx.x;
  int tot;
  const int p = block_prefix<kPWaves>(flag_of(m, d, i), wt, &tot);
  if (i <= range_len(m, d)) range_pre(m, d)[i] = boff[b] - boff[b0] + p;
}

// the merged id of the point at the node position whose lowest entry is e0
__device__ __forceinline__ int point_at(const MView &m, int e0) {
  return e0 < m.no_off[1] ? m.n1[e0] : m.pt_off[1] + 1 + m.pre_cre[e0];
}

// the merged id of concatenated tetra t (0-based) of group g
__device__ __forceinline__ int merged_tet(const MView &m, int t, int g) {
  if (g == 0) return t + 1;
  const int t0 = m.te_off[g], f0 = m.pre_ft[m.fa_off[g]];
  const u32 f = m.tetfirst[t];
  if (f != kNoEntry) return t0 + 1 + m.pre_ft[f] - f0;
  return t0 + (m.pre_ft[m.fa_off[g + 1]] - f0) + 1 + m.pre_int[t] - m.pre_int[t0];
}

// new_pt, src_pt, node_val
__global__ __launch_bounds__(kPBlock) void k_merge_points(MView m, MOut o, int n) {
  const int np0 = m.pt_off[1], ncre = m.pre_cre[m.En];
  const int stride = (int)gridDim.x * kPBlock;
  for (int i = (int)blockIdx.x * kPBlock + (int)threadIdx.x; i < n; i += stride) {
    if (i < m.P) {
      int id;
      bool mine = true; // this point is the merged point's source
      if (i < np0) {
        id = i + 1;
      } else {
        const u32 f = m.ptfirst[i];
        if (f == kNoEntry) {
          id = np0 + ncre + 1 + m.pre_unl[i];
        } else {
          const u32 e0 = m.posmin[m.n2[f]];
          id = point_at(m, (int)e0);
          mine = e0 == f;
        }
      }
      o.new_pt[i] = id;
      if (mine) o.src_pt[id - 1] = i + 1;
    }
    if (o.node_val && i < m.nnode) {
      const u32 e0 = m.posmin[i];
      int val = 0;
      if (e0 != kNoEntry) {
        val = point_at(m, (int)e0);
        const int holders = m.hold[i] + ((int)e0 < m.no_off[1] ? 1 : 0);
        if ((holders - 1) & 1) val = -val;
      }
      o.node_val[i] = val;
    }
  }
}

// new_tet, src_tet, tetv_out, mark_out, face_val (after k_merge_points: the corners go through new_pt)
__global__ __launch_bounds__(kPBlock) void k_merge_tetra(MView m, MOut o, int n) {
  const int stride = (int)gridDim.x * kPBlock;
  for (int i = (int)blockIdx.x * kPBlock + (int)threadIdx.x; i < n; i += stride) {
    if (i < m.T) {
      const int g = group_of(m.te_off, m.ngrp, i);
      const int id = merged_tet(m, i, g);
      if (o.new_tet) o.new_tet[i] = id;
      o.src_tet[id - 1] = i + 1;
      if (o.tetv_out) {
        const int4 v = m.tetv[(size_t)i * m.tstride];
        const int *np = o.new_pt + m.pt_off[g] - 1;
        o.tetv_out[id - 1] = make_int4(np[v.x], np[v.y], np[v.z], np[v.w]);
      }
      if (o.mark_out) o.mark_out[id - 1] = m.color[g];
    }
    if (o.face_val && i < m.nface) {
      const u32 e0 = m.fmin[i];
      int val = 0;
      if (e0 != kNoEntry) {
        int later = m.fcnt[i]; // the entries after the lowest: each negates the value
        if ((int)e0 < m.fa_off[1]) {
          val = m.f1[e0];
        } else {
          const int g = group_of(m.fa_off, m.ngrp, (int)e0), i1 = m.f1[e0];
          val = 12 * merged_tet(m, m.te_off[g] + i1 / 12 - 1, g) + i1 % 12;
          later--;
        }
        if (later & 1) val = -val;
      }
      o.face_val[i] = val;
    }
  }
}

int max_of(int a, int b) { return a > b ? a : b; }

} // namespace

int pmmg_merge_groups(hipStream_t s, const MergeArgs &a, MergeCache *c, char *msg, size_t msglen) {
  const int ngrp = a.ngrp;
  *a.np_out = 0;
  *a.ne_out = 0;
  std::vector<int> tab;
  MergeTotals tot;
  if (!merge_tables(ngrp, a.count, a.color, &tab, &tot, msg, msglen)) return 0;
  const int T = tot.ne, P = tot.np, Ef = tot.nface, En = tot.nnode, nnode = a.nnode, nface = a.nface;
  const size_t G = (size_t)ngrp + 1;

  // scratch (an allocation may synchronise the device: all of it ahead of the first kernel)
  const size_t nfirst = (size_t)P + T + nnode + nface, ncount = (size_t)nnode + nface;
  const size_t npre = (size_t)En + P + Ef + T + D_KINDS;
  int *words = get<int>(c->words, 4), *dtab = get<int>(c->tab, tab.size());
  u32 *firsts = get<u32>(c->firsts, nfirst);
  int *counts = get<int>(c->counts, ncount), *pre = get<int>(c->pre, npre);
  if (!words || !dtab || !firsts || !counts || !pre) {
    snprintf(msg, msglen, "merge_groups: out of device memory (scratch of %d tetra, %d points, %d groups)", T, P, ngrp);
    return 0;
  }
  // the four ranges of the counts, each one item longer than its entries, in blocks
  const int nb[D_KINDS] = {En / kPBlock + 1, P / kPBlock + 1, Ef / kPBlock + 1, T / kPBlock + 1};
  const int nblk = nb[0] + nb[1] + nb[2] + nb[3];
  if (!reserve(c->blocks, nblk, s, "merge_groups: out of device memory (block counts)", msg, msglen)) return 0;

  MView m;
  m.ngrp = ngrp;
  m.T = T, m.P = P, m.Ef = Ef, m.En = En;
  m.nnode = nnode, m.nface = nface;
  m.te_off = dtab, m.pt_off = dtab + G, m.fa_off = dtab + 2 * G, m.no_off = dtab + 3 * G, m.color = dtab + 4 * G;
  m.tetv = reinterpret_cast<const int4 *>(a.tetv);
  m.tstride = a.tstride;
  m.n1 = a.node_idx1, m.n2 = a.node_idx2, m.f1 = a.face_idx1, m.f2 = a.face_idx2;
  m.ptfirst = firsts, m.tetfirst = firsts + P, m.posmin = m.tetfirst + T, m.fmin = m.posmin + nnode;
  m.hold = counts, m.fcnt = counts + nnode;
  m.pre_cre = pre, m.pre_unl = m.pre_cre + En + 1, m.pre_ft = m.pre_unl + P + 1, m.pre_int = m.pre_ft + Ef + 1;
  m.b1 = nb[0], m.b2 = nb[0] + nb[1], m.b3 = nb[0] + nb[1] + nb[2];

  // the refusals: nothing is written to an output before they are known
  DEVCK(hipMemcpyAsync(dtab, tab.data(), tab.size() * sizeof(int), hipMemcpyHostToDevice, s));
  DEVCK(hipMemsetAsync(words, 0, 4 * sizeof(int), s));
  const int ncheck = max_of(T, max_of(En, Ef));
  hipLaunchKernelGGL(k_merge_check, dim3(grid_for(ncheck)), dim3(kPBlock), 0, s, m, ncheck, words);
  DEVCK(hipGetLastError());
  int f = 0;
  if (!read_word(s, words, &f, msg, msglen)) return 0;
  if (f & G_BADVERT) return refuse(msg, msglen, "merge_groups: a vertex id lies outside [1, np] of its group (nothing written)");
  if (f & G_BADNODE1)
    return refuse(msg, msglen, "merge_groups: a node index1 lies outside [1, np] of its group (nothing written)");
  if (f & G_BADNODE2) {
    snprintf(msg, msglen, "merge_groups: a node index2 lies outside [0, %d) (nothing written)", nnode);
    return 0;
  }
  if (f & G_BADFACE1)
    return refuse(msg, msglen, "merge_groups: a face index1 / 12 lies outside [1, ne] of its group (nothing written)");
  if (f & G_BADFACE2) {
    snprintf(msg, msglen, "merge_groups: a face index2 lies outside [0, %d) (nothing written)", nface);
    return 0;
  }

  // lowest entries, counts and places
  DEVCK(hipMemsetAsync(firsts, 0xff, sizeof(u32) * nfirst, s));
  DEVCK(hipMemsetAsync(counts, 0, sizeof(int) * ncount, s));
  const int nent = max_of(En, Ef);
  hipLaunchKernelGGL(k_merge_first, dim3(grid_for(nent)), dim3(kPBlock), 0, s, m, nent);
  hipLaunchKernelGGL(k_merge_pos, dim3(grid_for(En)), dim3(kPBlock), 0, s, m);
  hipLaunchKernelGGL(k_merge_counts, dim3(nblk), dim3(kPBlock), 0, s, m, c->blocks.btot.as<int>());
  DEVCK(hipGetLastError());
  if (!offsets(c->blocks, s, nblk, nullptr, msg, msglen)) return 0;
  hipLaunchKernelGGL(k_merge_prefix, dim3(nblk), dim3(kPBlock), 0, s, m, c->blocks.boff.as<int>());
  DEVCK(hipGetLastError());
  int ncre = 0, nunl = 0;
  DEVCK(hipMemcpyAsync(&ncre, m.pre_cre + En, sizeof(int), hipMemcpyDeviceToHost, s));
  DEVCK(hipMemcpyAsync(&nunl, m.pre_unl + P, sizeof(int), hipMemcpyDeviceToHost, s));
  DEVCK(hipStreamSynchronize(s));
  const int np = tab[G + 1] + ncre + nunl; // (at most P: every new point has a source of its own)
  *a.np_out = np;
  *a.ne_out = T;
  if (a.pt_cap < np) {
    snprintf(msg, msglen, "merge_groups: %d points exceed pt_cap = %lld (nothing written)", np, (long long)a.pt_cap);
    return 0;
  }
  if (np > 0 && !a.src_pt) return refuse(msg, msglen, "merge_groups: invalid arguments (src_pt is NULL)");

  // the maps, the tetra and the values
  const MOut o{a.new_pt, a.new_tet, a.src_pt, a.src_tet, reinterpret_cast<int4 *>(a.tetv_out),
               a.mark_out, a.node_val, a.face_val};
  const int npts = max_of(P, a.node_val ? nnode : 0), ntet = max_of(T, a.face_val ? nface : 0);
  hipLaunchKernelGGL(k_merge_points, dim3(grid_for(npts)), dim3(kPBlock), 0, s, m, o, npts);
  hipLaunchKernelGGL(k_merge_tetra, dim3(grid_for(ntet)), dim3(kPBlock), 0, s, m, o, ntet);
  DEVCK(hipGetLastError());
  DEVCK(hipStreamSynchronize(s));
  return 1;
}
