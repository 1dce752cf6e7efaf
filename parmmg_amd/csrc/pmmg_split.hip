// pmmg_split.hip — the sub-meshes and interface lists of a partition, on the
// device: what PMMG_split_eachGrp and PMMG_splitGrps_fillGroup
// (reference src/grpsplit_pmmg.c:819-1094, :1267-1445) leave for every colour
// of `part`, as a function of (tetv, adja, part) instead of a sequential loop.
//
// New order.  The tetra are sorted stably by colour (counting passes over the
// 8-bit digits of ngrp, per-tile histograms in LDS and wave-level ranks: any
// ngrp up to ne); a tetra's place n in that order, over all
// groups, is the index of every later pass, and a corner's place is 4 n + c.
// Ascending n is (colour, new tetra) order, so "first in the group" is a minimum
// over places and every list position is a prefix sum over n.
//
// First use of a vertex in a group.  Rounds of two launches.  In a round every
// corner that is not settled yet lowers its vertex's 64-bit word to
// (colour << 32 | place) (atomic_lower, pmmg_devutil.hpp); the next launch
// settles the corners whose colour is the word's (first[place] = the word's
// place) and resets the other array's word of
// every vertex that still has an unsettled corner.  Round r settles, at every
// vertex, its r-th lowest colour: interior vertices, the bulk, take one round,
// and a tetra whose corners are settled leaves a later round after one 16-byte
// read.  No kernel waits on another workgroup's store: the host reads one word
// per round.  The rounds of a call are the most colours that meet at one vertex.
//
// Counts.  k_split_mask leaves per tetra one word: which corners are first uses
// (points), which faces are owned interface faces, which faces make a face-list
// entry, which first-use corners already have a node position (run 1 of the node
// list), which face corners are their vertex's first interface occurrence in
// the owning colour (run 2).  Five prefix sums over n (block totals, one scan
// of the five tables laid end to end, block prefixes) give every entry its
// place; the per-group counts are differences at the colours' first places.
// No atomic touches a per-group or per-call word.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdio.h>

#include "pmmg_devutil.hpp"
#include "pmmg_split.hpp"

namespace {

typedef unsigned long long u64;
constexpr u64 kNone = ~0ULL;
constexpr int kNodeShift = 34; // 12 n + 11 < 2^34 for n < 2^29, and a colour below 2^29 stays in 63 bits

// the call's flag bits beside MESH_BADLINK and MESH_UNUSED of pmmg_devutil.hpp
enum { S_BADPART = 2, S_BADVERT = 16 };
// the call's words on the device
enum { W_FLAGS = 0, W_LEFT = 1, W_TOT = 2, W_COUNT = 8 };
// the kinds of entries counted per tetra, and their bits in a tetra's mask word
enum { K_PT = 0, K_FENT = 1, K_FOWN = 2, K_N1 = 3, K_N2 = 4, K_KINDS = 5 };
enum { M_PT = 0, M_FOWN = 4, M_FENT = 8, M_N1 = 12, M_N2 = 16 };

// MMG5_idir = {1,2,3}, {0,3,2}, {0,1,3}, {0,2,1}, two bits an entry: a constant wherever f and p are
__device__ __forceinline__ constexpr int idir(int f, int p) {
  return (int)((57u | 44u << 8 | 52u << 16 | 24u << 24) >> (8 * f + 2 * p) & 3u);
}

__device__ __forceinline__ int bits(unsigned int x) { return (int)__popc(x); }

// what the passes read of the mesh
struct SMesh : TetRows {
  int np;
  const int *part;
};

// The refusals, and the sort's values 1 .. ne.
__global__ __launch_bounds__(kPBlock) void k_split_check(SMesh m, int ngrp, int *iota, int *flags) {
  int bad = 0;
  const int stride = (int)gridDim.x * kPBlock;
  for (int k = (int)blockIdx.x * kPBlock + (int)threadIdx.x; k < m.ne; k += stride) {
    iota[k] = k + 1;
    if ((unsigned int)m.part[k] >= (unsigned int)ngrp) bad |= S_BADPART;
    const int4 v = m.tetv[(size_t)k * m.tstride];
    if (v.x <= 0) {
      bad |= MESH_UNUSED;
      continue;
    }
    const int vv[4] = {v.x, v.y, v.z, v.w};
    const int4 a = m.adja[(size_t)k * m.astride];
    const int lk[4] = {a.x, a.y, a.z, a.w};
#pragma unroll
    for (int f = 0; f < 4; f++) {
      if ((unsigned int)(vv[f] - 1) >= (unsigned int)m.np) bad |= S_BADVERT;
      if (lk[f] && !link_ok(lk[f], m.ne)) bad |= MESH_BADLINK;
    }
  }
  if (bad) atomicOr(flags, bad);
}

// ---- the stable sort by colour: one counting pass per 8-bit digit of the colour (pmmg_sort.hpp's scheme).
// A tile is kDigitTile consecutive keys; each wave of the tile's block takes kDigitItems chunks of 64
// consecutive keys.  hist is digit-major, hist[digit * ntile + tile], so its exclusive scan is the first
// output place of every (digit, tile).

constexpr int kDigitItems = 8, kDigitTile = kPBlock * kDigitItems;

// the lanes of the wave whose (valid) key has this lane's digit
__device__ __forceinline__ u64 same_digit(unsigned int d, bool ok) {
  u64 same = __ballot(ok);
#pragma unroll
  for (int b = 0; b < 8; b++) {
    const u64 bb = __ballot((d >> b) & 1u);
    same &= ((d >> b) & 1u) ? bb : ~bb;
  }
  return same;
}

__global__ __launch_bounds__(kPBlock) void k_split_digit_count(int ne, int shift, int ntile, const int *keys, int *hist) {
  static_assert(kPBlock == 256, "one thread per digit");
  __shared__ int h[256];
  const int t = threadIdx.x, w = t >> 6, lane = t & 63;
  const u64 below = (1ULL << lane) - 1ULL;
  for (int tile = blockIdx.x; tile < ntile; tile += gridDim.x) {
    h[t] = 0;
    __syncthreads();
    const long long base = (long long)tile * kDigitTile + w * (kDigitTile / kPWaves);
#pragma unroll
    for (int j = 0; j < kDigitItems; j++) {
      const long long e = base + j * 64 + lane;
      const bool ok = e < ne;
      const unsigned int d = ok ? ((unsigned int)keys[e] >> shift) & 255u : 0u;
      const u64 same = same_digit(d, ok);
      if (ok && !(same & below)) atomicAdd(&h[d], __popcll(same)); // (LDS; one lane per wave, chunk and digit)
    }
    __syncthreads();
    hist[(size_t)t * ntile + tile] = h[t];
    __syncthreads();
  }
}

__global__ __launch_bounds__(kPBlock) void k_split_digit_scatter(int ne, int shift, int ntile, const int *off,
                                                                 const int *kin, const int *vin, int *kout, int *vout) {
  __shared__ int wdig[kPWaves][256]; // a wave's count per digit, then the first output place of its keys of the digit
  const int t = threadIdx.x, w = t >> 6, lane = t & 63;
  const u64 below = (1ULL << lane) - 1ULL;
  for (int tile = blockIdx.x; tile < ntile; tile += gridDim.x) {
#pragma unroll
    for (int q = 0; q < kPWaves; q++) wdig[q][t] = 0;
    __syncthreads();
    const long long base = (long long)tile * kDigitTile + w * (kDigitTile / kPWaves);
    int key[kDigitItems], val[kDigitItems], rk[kDigitItems];
#pragma unroll
    for (int j = 0; j < kDigitItems; j++) {
      const long long e = base + j * 64 + lane;
      key[j] = e < ne ? kin[e] : 0;
      val[j] = e < ne ? vin[e] : 0;
    }
#pragma unroll
    for (int j = 0; j < kDigitItems; j++) {
      const bool ok = base + j * 64 + lane < ne;
      const unsigned int d = ((unsigned int)key[j] >> shift) & 255u;
      const u64 same = same_digit(d, ok);
      const int r = __popcll(same & below);
      const int prior = wdig[w][d]; // (the wave's own counter: read by every lane before its first lane writes it)
      rk[j] = prior + r;
      __builtin_amdgcn_wave_barrier();
      if (ok && r == 0) wdig[w][d] = prior + __popcll(same);
      __builtin_amdgcn_wave_barrier();
    }
    __syncthreads();
    int acc = off[(size_t)t * ntile + tile];
#pragma unroll
    for (int q = 0; q < kPWaves; q++) {
      const int c = wdig[q][t];
      wdig[q][t] = acc;
      acc += c;
    }
    __syncthreads();
#pragma unroll
    for (int j = 0; j < kDigitItems; j++) {
      if (base + j * 64 + lane < ne) {
        const int p = wdig[w][((unsigned int)key[j] >> shift) & 255u] + rk[j];
        kout[p] = key[j];
        vout[p] = val[j];
      }
    }
    __syncthreads(); // the tile's LDS is free for the next tile
  }
}

// pos[old tetra] = its new place; teoff[g] = the first place of colour g (of the next colour that has tetra, or
// ne).  The thread of a colour's first tetra writes the entries of the empty colours before it as well.
__global__ __launch_bounds__(kPBlock) void k_split_places(int ne, int ngrp, const int *skey, const int *old_tet,
                                                          int *pos, int *teoff) {
  const int stride = (int)gridDim.x * kPBlock;
  for (int n = (int)blockIdx.x * kPBlock + (int)threadIdx.x; n < ne; n += stride) {
    pos[old_tet[n] - 1] = n;
    const int g = skey[n], prev = n ? skey[n - 1] : -1;
    for (int c = prev + 1; c <= g; c++) teoff[c] = n;
    if (n == ne - 1)
      for (int c = g + 1; c <= ngrp; c++) teoff[c] = ne;
  }
}

// A round's first launch: the unsettled corners lower their vertices' words.
__global__ __launch_bounds__(kPBlock) void k_split_first_min(SMesh m, const int *skey, const int *old_tet,
                                                             const int4 *first, u64 *cur) {
  const int stride = (int)gridDim.x * kPBlock;
  for (int n = (int)blockIdx.x * kPBlock + (int)threadIdx.x; n < m.ne; n += stride) {
    const int4 fr = first[n];
    if ((fr.x | fr.y | fr.z | fr.w) >= 0) continue;
    const int4 v = m.tetv[(size_t)(old_tet[n] - 1) * m.tstride];
    const int vv[4] = {v.x, v.y, v.z, v.w}, ff[4] = {fr.x, fr.y, fr.z, fr.w};
    const u64 key = ((u64)(unsigned int)skey[n] << 32) | (u64)(unsigned int)(4 * n);
#pragma unroll
    for (int c = 0; c < 4; c++)
      if (ff[c] < 0) atomic_lower(&cur[vv[c] - 1], key + (u64)c);
  }
}

// A round's second launch: a corner whose colour is its vertex's word is settled; the vertex of one that is not
// gets its word of the next round reset.  *left: a plain store of 1 by whoever stays unsettled.
__global__ __launch_bounds__(kPBlock) void k_split_first_settle(SMesh m, const int *skey, const int *old_tet,
                                                                int4 *first, const u64 *cur, u64 *nxt, int *left) {
  bool l = false;
  const int stride = (int)gridDim.x * kPBlock;
  for (int n = (int)blockIdx.x * kPBlock + (int)threadIdx.x; n < m.ne; n += stride) {
    const int4 fr = first[n];
    if ((fr.x | fr.y | fr.z | fr.w) >= 0) continue;
    const int4 v = m.tetv[(size_t)(old_tet[n] - 1) * m.tstride];
    const int vv[4] = {v.x, v.y, v.z, v.w};
    int ff[4] = {fr.x, fr.y, fr.z, fr.w};
    const unsigned int g = (unsigned int)skey[n];
#pragma unroll
    for (int c = 0; c < 4; c++) {
      if (ff[c] >= 0) continue;
      const u64 w = cur[vv[c] - 1];
      if ((unsigned int)(w >> 32) == g) {
        ff[c] = (int)(unsigned int)(w & 0xffffffffu);
      } else {
        nxt[vv[c] - 1] = kNone;
        l = true;
      }
    }
    first[n] = make_int4(ff[0], ff[1], ff[2], ff[3]);
  }
  if (l) *left = 1;
}

// Per vertex without an old position: the lowest (colour, 12 n + 3 f + p) over the corners of the faces towards
// another colour: its owner and its rank among the owner's new interface nodes.
__global__ __launch_bounds__(kPBlock) void k_split_node_min(SMesh m, const int *skey, const int *old_tet,
                                                            const int *node_pos, u64 *nmin) {
  const int stride = (int)gridDim.x * kPBlock;
  for (int n = (int)blockIdx.x * kPBlock + (int)threadIdx.x; n < m.ne; n += stride) {
    const int k = old_tet[n] - 1, g = skey[n];
    const int4 a = m.adja[(size_t)k * m.astride];
    const int lk[4] = {a.x, a.y, a.z, a.w};
    int out = 0;
#pragma unroll
    for (int f = 0; f < 4; f++)
      if (lk[f] && m.part[lk[f] / 4 - 1] != g) out |= 1 << f;
    if (!out) continue;
    const int4 v = m.tetv[(size_t)k * m.tstride];
    const int vv[4] = {v.x, v.y, v.z, v.w};
    const u64 base = ((u64)(unsigned int)g << kNodeShift) | (u64)(12 * (long long)n);
#pragma unroll
    for (int f = 0; f < 4; f++) {
      if (!(out >> f & 1)) continue;
#pragma unroll
      for (int p = 0; p < 3; p++) {
        const int x = vv[idir(f, p)] - 1;
        if (!node_pos || node_pos[x] < 0) atomic_lower(&nmin[x], base + (u64)(3 * f + p));
      }
    }
  }
}

// The mask word of every new tetra (the header of this file).
__global__ __launch_bounds__(kPBlock) void k_split_mask(SMesh m, const int *skey, const int *old_tet, const int4 *first,
                                                        const int *node_pos, const int *face_old, const u64 *nmin,
                                                        unsigned int *mask) {
  const int stride = (int)gridDim.x * kPBlock;
  for (int n = (int)blockIdx.x * kPBlock + (int)threadIdx.x; n < m.ne; n += stride) {
    const int k = old_tet[n] - 1, g = skey[n];
    const int4 v = m.tetv[(size_t)k * m.tstride];
    const int vv[4] = {v.x, v.y, v.z, v.w};
    const int4 a = m.adja[(size_t)k * m.astride];
    const int lk[4] = {a.x, a.y, a.z, a.w};
    const int4 fr = first[n];
    const int ff[4] = {fr.x, fr.y, fr.z, fr.w};
    unsigned int w = 0;
#pragma unroll
    for (int c = 0; c < 4; c++) {
      if (ff[c] != 4 * n + c) continue;
      w |= 1u << (M_PT + c);
      const int x = vv[c] - 1;
      bool has = node_pos && node_pos[x] >= 0;
      if (!has) {
        const u64 o = nmin[x];
        has = o != kNone && (int)(o >> kNodeShift) < g;
      }
      if (has) w |= 1u << (M_N1 + c);
    }
    const u64 base = ((u64)(unsigned int)g << kNodeShift) | (u64)(12 * (long long)n);
#pragma unroll
    for (int f = 0; f < 4; f++) {
      if (!lk[f]) {
        if (face_old && face_old[4 * (size_t)k + f] >= 0) w |= 1u << (M_FENT + f);
        continue;
      }
      const int gj = m.part[lk[f] / 4 - 1];
      if (gj == g) continue;
      w |= 1u << (M_FENT + f);
      if (gj > g) w |= 1u << (M_FOWN + f);
#pragma unroll
      for (int p = 0; p < 3; p++)
        if (nmin[vv[idir(f, p)] - 1] == base + (u64)(3 * f + p)) w |= 1u << (M_N2 + 3 * f + p);
    }
    mask[n] = w;
  }
}

// The five counts of a tetra's mask prefixed over the block (three packed prefixes: a block's sum is at most 1024).
__device__ __forceinline__ void five_prefix(unsigned int w, int *wt, int pre[K_KINDS], int tot[K_KINDS]) {
  const int c[K_KINDS + 1] = {bits(w >> M_PT & 15u), bits(w >> M_FENT & 15u), bits(w >> M_FOWN & 15u),
                              bits(w >> M_N1 & 15u), bits(w >> M_N2 & 4095u), 0};
#pragma unroll
  for (int i = 0; i < K_KINDS; i += 2) {
    int t;
    const int p = block_prefix<kPWaves>(c[i] | (c[i + 1] << 16), wt, &t);
    pre[i] = p & 0xffff;
    tot[i] = t & 0xffff;
    if (i + 1 < K_KINDS) {
      pre[i + 1] = p >> 16;
      tot[i + 1] = t >> 16;
    }
    __syncthreads();
  }
}

// btot[kind * nblk + b] = the entries of kind `kind` in block b = new tetra 256 b .. 256 b + 255
__global__ __launch_bounds__(kPBlock) void k_split_block_counts(int ne, int nblk, const unsigned int *mask, int *btot) {
  __shared__ int wt[kPWaves];
  const int n = (int)blockIdx.x * kPBlock + (int)threadIdx.x;
  int pre[K_KINDS], tot[K_KINDS];
  five_prefix(n < ne ? mask[n] : 0u, wt, pre, tot);
  if (threadIdx.x < K_KINDS) {
    int t = tot[0];
#pragma unroll
    for (int i = 1; i < K_KINDS; i++) t = (int)threadIdx.x == i ? tot[i] : t;
    btot[(size_t)threadIdx.x * nblk + blockIdx.x] = t;
  }
}

// pre[kind * (ne + 1) + n] = the entries of that kind before new tetra n; [ne]: all of them
__global__ __launch_bounds__(kPBlock) void k_split_prefix(int ne, int nblk, const unsigned int *mask, const int *boff,
                                                          int *pre_out) {
  __shared__ int wt[kPWaves];
  const int n = (int)blockIdx.x * kPBlock + (int)threadIdx.x;
  int pre[K_KINDS], tot[K_KINDS];
  five_prefix(n < ne ? mask[n] : 0u, wt, pre, tot);
  if (n >= ne) return;
#pragma unroll
  for (int i = 0; i < K_KINDS; i++) {
    const int b = boff[(size_t)i * nblk + blockIdx.x] - boff[(size_t)i * nblk];
    pre_out[(size_t)i * (ne + 1) + n] = b + pre[i];
    if (n == ne - 1) pre_out[(size_t)i * (ne + 1) + ne] = b + tot[i];
  }
}

// table[g] = {ne, np, nface, nnode} of group g; tot[kind] = the entries of every kind
__global__ __launch_bounds__(kPBlock) void k_split_table(int ne, int ngrp, const int *teoff, const int *pre, int4 *table,
                                                         int *tot) {
  const int g = (int)blockIdx.x * kPBlock + (int)threadIdx.x;
  if (g > ngrp) return;
  const size_t S = (size_t)ne + 1;
  if (g == ngrp) {
    for (int i = 0; i < K_KINDS; i++) tot[i] = pre[i * S + ne];
    return;
  }
  const int a = teoff[g], b = teoff[g + 1];
  table[g] = make_int4(b - a, pre[K_PT * S + b] - pre[K_PT * S + a], pre[K_FENT * S + b] - pre[K_FENT * S + a],
                       (pre[K_N1 * S + b] - pre[K_N1 * S + a]) + (pre[K_N2 * S + b] - pre[K_N2 * S + a]));
}

// the id, in its group, of the point that the corner `q` (a place 4 n' + c', a first use) made; p0: the points
// before the group
__device__ __forceinline__ int point_id(int q, const unsigned int *mask, const int *pre_pt, int p0) {
  const int n1 = q >> 2, c1 = q & 3;
  return pre_pt[n1] + __popc(mask[n1] >> M_PT & ((1u << c1) - 1u)) - p0 + 1;
}

// new_tet, tetv_out, adja_out, tet8_out
__global__ __launch_bounds__(kPBlock) void k_split_emit(SMesh m, const int *skey, const int *old_tet, const int *pos,
                                                        const int *teoff, const int4 *first, const unsigned int *mask,
                                                        const int *pre_pt, int *new_tet, int4 *tetv_out,
                                                        int4 *adja_out, int4 *tet8_out) {
  const int stride = (int)gridDim.x * kPBlock;
  for (int n = (int)blockIdx.x * kPBlock + (int)threadIdx.x; n < m.ne; n += stride) {
    const int k = old_tet[n] - 1, g = skey[n], n0 = teoff[g];
    if (new_tet) new_tet[k] = n - n0 + 1;
    if (!tetv_out && !adja_out && !tet8_out) continue;
    const int p0 = pre_pt[n0];
    const int4 fr = first[n];
    const int4 v = make_int4(point_id(fr.x, mask, pre_pt, p0), point_id(fr.y, mask, pre_pt, p0),
                             point_id(fr.z, mask, pre_pt, p0), point_id(fr.w, mask, pre_pt, p0));
    const int4 a = m.adja[(size_t)k * m.astride];
    int lk[4] = {a.x, a.y, a.z, a.w};
#pragma unroll
    for (int f = 0; f < 4; f++) {
      if (!lk[f]) continue;
      const int j = lk[f] / 4 - 1;
      lk[f] = m.part[j] == g ? 4 * (pos[j] - n0 + 1) + (lk[f] & 3) : 0;
    }
    const int4 l = make_int4(lk[0], lk[1], lk[2], lk[3]);
    if (tetv_out) tetv_out[n] = v;
    if (adja_out) adja_out[n] = l;
    if (tet8_out) {
      tet8_out[2 * (size_t)n] = v;
      tet8_out[2 * (size_t)n + 1] = l;
    }
  }
}

// old_pt, the face lists, and the second run of the node lists with the positions it gives (vpos)
__global__ __launch_bounds__(kPBlock) void k_split_lists(SMesh m, const int *skey, const int *old_tet, const int *pos,
                                                         const int *teoff, const int4 *first, const unsigned int *mask,
                                                         const int *pre, const int *face_old, int nnode0, int nface0,
                                                         int *old_pt, int *face_idx1, int *face_idx2, int *node_idx1,
                                                         int *node_idx2, int *vpos) {
  const size_t S = (size_t)m.ne + 1;
  const int *pre_pt = pre + K_PT * S, *pre_fe = pre + K_FENT * S, *pre_fo = pre + K_FOWN * S, *pre_n1 = pre + K_N1 * S,
            *pre_n2 = pre + K_N2 * S;
  const int stride = (int)gridDim.x * kPBlock;
  for (int n = (int)blockIdx.x * kPBlock + (int)threadIdx.x; n < m.ne; n += stride) {
    const unsigned int w = mask[n];
    if (!w) continue;
    const int k = old_tet[n] - 1, g = skey[n], n0 = teoff[g], t = n - n0 + 1;
    const int4 v = m.tetv[(size_t)k * m.tstride];
    const int vv[4] = {v.x, v.y, v.z, v.w};
    int at = pre_pt[n];
#pragma unroll
    for (int c = 0; c < 4; c++)
      if (w >> (M_PT + c) & 1u) old_pt[at++] = vv[c];
    if (!(w >> M_FENT & 15u)) continue; // (no face entry: no new interface node either)
    const int4 a = m.adja[(size_t)k * m.astride];
    const int lk[4] = {a.x, a.y, a.z, a.w};
    at = pre_fe[n];
    const int own0 = nface0 + pre_fo[n];
#pragma unroll
    for (int f = 0; f < 4; f++) {
      if (!(w >> (M_FENT + f) & 1u)) continue;
      int iploc, num;
      if (!lk[f]) {
        const int fo = face_old[4 * (size_t)k + f];
        iploc = fo % 3;
        num = fo / 3;
      } else if (w >> (M_FOWN + f) & 1u) {
        iploc = 0;
        num = own0 + __popc(w >> M_FOWN & ((1u << f) - 1u));
      } else { // the lower colour's side owns the face: its number, and its first vertex in this side's order
        const int j = lk[f] / 4 - 1, i = lk[f] & 3, nj = pos[j];
        num = nface0 + pre_fo[nj] + __popc(mask[nj] >> M_FOWN & ((1u << i) - 1u));
        const int4 u = m.tetv[(size_t)j * m.tstride];
        const int ip = i == 0 ? u.y : u.x; // u[MMG5_idir[i][0]]
        iploc = vv[idir(f, 1)] == ip ? 1 : (vv[idir(f, 2)] == ip ? 2 : 0);
      }
      face_idx1[at] = 12 * t + 3 * f + iploc;
      face_idx2[at] = num;
      at++;
    }
    if (!(w >> M_N2 & 4095u)) continue;
    const int4 fr = first[n];
    const int ff[4] = {fr.x, fr.y, fr.z, fr.w};
    const int p0 = pre_pt[n0];
    at = pre_n1[teoff[g + 1]] + pre_n2[n]; // after the first runs up to this group and the second runs before n
#pragma unroll
    for (int b = 0; b < 12; b++) {
      if (!(w >> (M_N2 + b) & 1u)) continue;
      const int c = idir(b / 3, b % 3);
      node_idx1[at] = point_id(ff[c], mask, pre_pt, p0);
      node_idx2[at] = nnode0 + at + 1; // the reference's nitem + 1, nitem counting appended entries
      vpos[vv[c] - 1] = nnode0 + at + 1;
      at++;
    }
  }
}

// the first run of the node lists: the points of a group that came with a position or got one from a lower colour
__global__ __launch_bounds__(kPBlock) void k_split_nodes_old(SMesh m, const int *skey, const int *old_tet,
                                                             const int *teoff, const unsigned int *mask, const int *pre,
                                                             const int *node_pos, const int *vpos, int *node_idx1,
                                                             int *node_idx2) {
  const size_t S = (size_t)m.ne + 1;
  const int *pre_pt = pre + K_PT * S, *pre_n1 = pre + K_N1 * S, *pre_n2 = pre + K_N2 * S;
  const int stride = (int)gridDim.x * kPBlock;
  for (int n = (int)blockIdx.x * kPBlock + (int)threadIdx.x; n < m.ne; n += stride) {
    const unsigned int w = mask[n];
    if (!(w >> M_N1 & 15u)) continue;
    const int n0 = teoff[skey[n]];
    const int4 v = m.tetv[(size_t)(old_tet[n] - 1) * m.tstride];
    const int vv[4] = {v.x, v.y, v.z, v.w};
    int at = pre_n2[n0] + pre_n1[n]; // after the second runs of the lower colours and the first runs before n
    int id = pre_pt[n] - pre_pt[n0];
#pragma unroll
    for (int c = 0; c < 4; c++) {
      if (!(w >> (M_PT + c) & 1u)) continue;
      id++;
      if (!(w >> (M_N1 + c) & 1u)) continue;
      const int x = vv[c] - 1;
      node_idx1[at] = id;
      node_idx2[at] = node_pos && node_pos[x] >= 0 ? node_pos[x] : vpos[x];
      at++;
    }
  }
}

int bits_of(int ngrp) {
  int b = 1;
  while (b < 31 && (1LL << b) < ngrp) b++;
  return b;
}

} // namespace

int pmmg_split_groups(hipStream_t s, const SplitArgs &a, SplitCache *c, char *msg, size_t msglen) {
  const int ne = a.m.ne, ngrp = a.ngrp, np = a.np;
  c->rounds = 0;
  for (int g = 0; g < ngrp; g++) a.count[g] = pmmg_hip_split_count{0, 0, 0, 0};
  *a.nnode_end = a.nnode0;
  *a.nface_end = a.nface0;
  if (ne == 0) return 1;
  const int nblk = (ne + kPBlock - 1) / kPBlock, grid = grid_for(ne);
  const size_t S = (size_t)ne + 1;

  // scratch (an allocation may synchronise the device: all of it ahead of the first kernel)
  int *words = get<int>(c->words, W_COUNT), *iota = get<int>(c->iota, (size_t)ne), *skey = get<int>(c->skey, (size_t)ne);
  int *pos = get<int>(c->pos, (size_t)ne), *teoff = get<int>(c->teoff, (size_t)ngrp + 1);
  int4 *first = get<int4>(c->first, (size_t)ne);
  u64 *vmin[2] = {get<u64>(c->vmin[0], (size_t)np), get<u64>(c->vmin[1], (size_t)np)};
  u64 *nmin = get<u64>(c->nmin, (size_t)np);
  int *vpos = get<int>(c->vpos, (size_t)np);
  unsigned int *mask = get<unsigned int>(c->mask, (size_t)ne);
  int *pre = get<int>(c->pre, K_KINDS * S);
  int4 *table = get<int4>(c->table, (size_t)ngrp);
  const int npass = (bits_of(ngrp) + 7) / 8, ntile = (ne + kDigitTile - 1) / kDigitTile;
  int *tmpk = npass > 1 ? get<int>(c->sort_tmp, 2 * (size_t)ne) : iota, *tmpv = npass > 1 ? tmpk + ne : iota;
  void *sort_tmp = tmpk;
  if (!words || !iota || !skey || !pos || !teoff || !first || !vmin[0] || !vmin[1] || !nmin || !vpos || !mask || !pre ||
      !table || !sort_tmp) {
    snprintf(msg, msglen, "split_groups: out of device memory (scratch of %d tetra, %d points, %d groups)", ne, np, ngrp);
    return 0;
  }
  if (!reserve(c->blocks, K_KINDS * nblk, s, "split_groups: out of device memory (block counts)", msg, msglen)) return 0;
  if (!reserve(c->digits, 256 * ntile, s, "split_groups: out of device memory (digit counts)", msg, msglen)) return 0;

  const SMesh m{rows_of(a.m), np, a.part};

  // the refusals: nothing is written to an output before they are known
  DEVCK(hipMemsetAsync(words, 0, W_COUNT * sizeof(int), s));
  hipLaunchKernelGGL(k_split_check, dim3(grid), dim3(kPBlock), 0, s, m, ngrp, iota, words + W_FLAGS);
  DEVCK(hipGetLastError());
  int f = 0;
  if (!read_word(s, words + W_FLAGS, &f, msg, msglen)) return 0;
  if (f & S_BADPART) {
    snprintf(msg, msglen, "split_groups: a part value lies outside [0, %d) (nothing written)", ngrp);
    return 0;
  }
  if (f & MESH_UNUSED) {
    snprintf(msg, msglen, "split_groups: an unused tetra (v[0] <= 0): the mesh must be packed (nothing written)");
    return 0;
  }
  if (f & MESH_BADLINK) {
    snprintf(msg, msglen, "split_groups: an adja entry lies outside [4, 4*%d+3] (nothing written)", ne);
    return 0;
  }
  if (f & S_BADVERT) {
    snprintf(msg, msglen, "split_groups: a vertex id lies outside [1, %d] (nothing written)", np);
    return 0;
  }

  // the new order
  const int *kin = a.part, *vin = iota;
  const int tgrid = ntile < kPMaxBlocks ? ntile : kPMaxBlocks;
  for (int i = 0; i < npass; i++) { // (the last pass writes skey and old_tet; the passes before it alternate)
    const bool fin = (npass - 1 - i) % 2 == 0;
    int *kout = fin ? skey : tmpk, *vout = fin ? a.old_tet : tmpv;
    hipLaunchKernelGGL(k_split_digit_count, dim3(tgrid), dim3(kPBlock), 0, s, ne, 8 * i, ntile, kin,
                       c->digits.btot.as<int>());
    DEVCK(hipGetLastError());
    if (!offsets(c->digits, s, 256 * ntile, nullptr, msg, msglen)) return 0;
    hipLaunchKernelGGL(k_split_digit_scatter, dim3(tgrid), dim3(kPBlock), 0, s, ne, 8 * i, ntile,
                       c->digits.boff.as<int>(), kin, vin, kout, vout);
    DEVCK(hipGetLastError());
    kin = kout;
    vin = vout;
  }
  hipLaunchKernelGGL(k_split_places, dim3(grid), dim3(kPBlock), 0, s, ne, ngrp, skey, a.old_tet, pos, teoff);
  DEVCK(hipGetLastError());

  // first uses
  DEVCK(hipMemsetAsync(first, 0xff, sizeof(int4) * (size_t)ne, s));
  DEVCK(hipMemsetAsync(vmin[0], 0xff, sizeof(u64) * (size_t)np, s));
  DEVCK(hipMemsetAsync(nmin, 0xff, sizeof(u64) * (size_t)np, s));
  for (int r = 0;; r++) {
    if (r > ngrp) { // (round r settles a vertex's r-th lowest colour)
      snprintf(msg, msglen, "split_groups: first uses not settled after %d rounds", r);
      return 0;
    }
    u64 *cur = vmin[r & 1], *nxt = vmin[(r + 1) & 1];
    DEVCK(hipMemsetAsync(words + W_LEFT, 0, sizeof(int), s));
    hipLaunchKernelGGL(k_split_first_min, dim3(grid), dim3(kPBlock), 0, s, m, skey, a.old_tet, first, cur);
    hipLaunchKernelGGL(k_split_first_settle, dim3(grid), dim3(kPBlock), 0, s, m, skey, a.old_tet, first, cur, nxt,
                       words + W_LEFT);
    DEVCK(hipGetLastError());
    c->rounds++;
    int left = 0;
    if (!read_word(s, words + W_LEFT, &left, msg, msglen)) return 0;
    if (!left) break;
  }

  // counts and places
  int *btot = c->blocks.btot.as<int>();
  const int *boff = c->blocks.boff.as<int>();
  hipLaunchKernelGGL(k_split_node_min, dim3(grid), dim3(kPBlock), 0, s, m, skey, a.old_tet, a.node_pos, nmin);
  hipLaunchKernelGGL(k_split_mask, dim3(grid), dim3(kPBlock), 0, s, m, skey, a.old_tet, first, a.node_pos, a.face_old,
                     nmin, mask);
  hipLaunchKernelGGL(k_split_block_counts, dim3(nblk), dim3(kPBlock), 0, s, ne, nblk, mask, btot);
  DEVCK(hipGetLastError());
  if (!offsets(c->blocks, s, K_KINDS * nblk, nullptr, msg, msglen)) return 0;
  hipLaunchKernelGGL(k_split_prefix, dim3(nblk), dim3(kPBlock), 0, s, ne, nblk, mask, boff, pre);
  hipLaunchKernelGGL(k_split_table, dim3((ngrp + 1 + kPBlock - 1) / kPBlock), dim3(kPBlock), 0, s, ne, ngrp, teoff, pre,
                     table, words + W_TOT);
  hipLaunchKernelGGL(k_split_emit, dim3(grid), dim3(kPBlock), 0, s, m, skey, a.old_tet, pos, teoff, first, mask,
                     pre + K_PT * S, a.new_tet, reinterpret_cast<int4 *>(a.tetv_out),
                     reinterpret_cast<int4 *>(a.adja_out), reinterpret_cast<int4 *>(a.tet8_out));
  DEVCK(hipGetLastError());
  static_assert(sizeof(pmmg_hip_split_count) == sizeof(int4), "the table's rows are pmmg_hip_split_count");
  int tot[K_KINDS];
  DEVCK(hipMemcpyAsync(a.count, table, sizeof(int4) * (size_t)ngrp, hipMemcpyDeviceToHost, s));
  DEVCK(hipMemcpyAsync(tot, words + W_TOT, sizeof(tot), hipMemcpyDeviceToHost, s));
  DEVCK(hipStreamSynchronize(s));
  const int64_t nnode = (int64_t)tot[K_N1] + tot[K_N2];
  if ((int64_t)a.nnode0 + nnode > INT32_MAX || (int64_t)a.nface0 + tot[K_FOWN] > INT32_MAX) {
    snprintf(msg, msglen, "split_groups: the positions exceed an int (%lld node entries after %d, %d faces after %d)",
             (long long)nnode, a.nnode0, tot[K_FOWN], a.nface0);
    return 0;
  }
  *a.nnode_end = a.nnode0 + (int)nnode;
  *a.nface_end = a.nface0 + tot[K_FOWN];
  if (a.pt_cap < tot[K_PT] || a.face_cap < tot[K_FENT] || a.node_cap < nnode) {
    snprintf(msg, msglen,
             "split_groups: %d points, %d face entries, %lld node entries exceed pt_cap = %lld, face_cap = %lld, "
             "node_cap = %lld (nothing written to old_pt or the lists)",
             tot[K_PT], tot[K_FENT], (long long)nnode, (long long)a.pt_cap, (long long)a.face_cap,
             (long long)a.node_cap);
    return 0;
  }
  if ((tot[K_PT] && !a.old_pt) || (tot[K_FENT] && (!a.face_idx1 || !a.face_idx2)) ||
      (nnode && (!a.node_idx1 || !a.node_idx2))) {
    snprintf(msg, msglen, "split_groups: invalid arguments (a list with entries is NULL)");
    return 0;
  }

  // the lists
  hipLaunchKernelGGL(k_split_lists, dim3(grid), dim3(kPBlock), 0, s, m, skey, a.old_tet, pos, teoff, first, mask, pre,
                     a.face_old, a.nnode0, a.nface0, a.old_pt, a.face_idx1, a.face_idx2, a.node_idx1, a.node_idx2, vpos);
  hipLaunchKernelGGL(k_split_nodes_old, dim3(grid), dim3(kPBlock), 0, s, m, skey, a.old_tet, teoff, mask, pre,
                     a.node_pos, vpos, a.node_idx1, a.node_idx2);
  DEVCK(hipGetLastError());
  DEVCK(hipStreamSynchronize(s));
  return 1;
}
