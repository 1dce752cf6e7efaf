// pmmg_contig.hip — the subgroups of a partition and their fix, on the device
// (DESIGN.md §11).
//
// A subgroup is a connected component of the tetra adjacency restricted to one
// colour: what PMMG_check_part_contiguity (reference src/metis_pmmg.c:312),
// PMMG_check_grps_contiguity (:446) and PMMG_check_contiguity
// (src/moveinterfaces_pmmg.c:309) count with ascending sweeps, and what
// PMMG_fix_contiguity (:475-523) lists by BFS and moves.
//
// Labelling: hook and flatten over kernel launches, on two arrays.  P[k] is a
// tetra's parent, never above k; L[k] is its root at the start of a round.
// A hooking round reads L only and lowers, in P, the parent of the higher of
// two roots joined by a same-colour link (atomicMin, agent scope, no return):
// a round sees nothing of its own hooks, and what it leaves, P[R] = the lowest
// root among R and its neighbouring roots, does not depend on the
// interleaving.  P is then flattened in place by pointer jumping until every
// tetra points at its root, and the pass that finds it flat has written L.
// No kernel waits for another workgroup's store: a value read at P[x] during
// a flatten pass, fresh or stale, is an ancestor of x, every chase ends at a
// root that the pass does not modify, and what a pass left undone is seen by
// the host between two launches, where memory is coherent.  Round 1 is fused
// into the initial pass (a tetra's parent = its lowest same-colour neighbour
// below it: what the atomicMin of a first round over singleton trees leaves).
// The bound.  A root R that survives a round is the minimum of its
// neighbouring roots, and each of those, R', was hooked to the lowest of its
// own neighbouring roots, which is R or lower.  Either all went to R itself,
// and R absorbed at least one root; or one went below R, R's tree then touches
// a tree with a lower root, and R is hooked in the next round.  So a root that
// survives two consecutive rounds absorbed a root of its own in the first,
// different survivors different ones: the roots of a subgroup at least halve
// every two rounds, and with the idle last round there are at most
// 2 ceil(log2 ne) + 1 rounds (2 for ne = 1).  One round does not halve them (a
// star with a high centre keeps every leaf; trees built like Fibonacci words
// need about 1.44 log2 ne rounds: tests/contig_ref.py).  The rounds and the
// labels, the subgroup's lowest tetra, are the same in every run; only the
// number of flatten passes depends on the interleaving.
//
// Table: heads are the tetra with L[k] == k; block counts and a scan give
// every head its row in ascending order.  Sizes are counted per block in an
// LDS table (CountTable, pmmg_devutil.hpp) and leave once per block and
// distinct row (a wave whose 64 tetra share a row adds 64 with one lane);
// `exit` is a minimum over the rim (atomic_lower).  No per-tetra atomic goes to
// a per-subgroup word.
#include <hip/hip_runtime.h>
#include <limits.h>
#include <stdint.h>
#include <stdio.h>

#include <vector>

#include "pmmg_contig.hpp"
#include "pmmg_contig_decide.hpp"
#include "pmmg_devutil.hpp"

static_assert(sizeof(ContigSub) == sizeof(pmmg_hip_subgroup), "the table's rows are pmmg_hip_subgroup");

namespace {

constexpr int kCJumps = 16; // parents followed per tetra and flatten pass
// the size table of a block: 1024 slots, 8 tried before a count goes to the row's word directly
typedef CountTable<1024, 8> SizeTable;

// the call's own flag bit, beside the MESH_ bits of pmmg_devutil.hpp
enum { C_BADPART = 2 };
// the call's words on the device
enum { W_FLAGS = 0, W_PASS = 1, W_VMAX = 2, W_COUNT = 4 };

// Round 1 and the checks.  P[k] = -1 for an unused row, else the lowest same-colour neighbour below k, or k.
// flags: a link out of range, a colour outside [0, ncolor), an unused row seen.
__global__ __launch_bounds__(kPBlock) void k_contig_init(int ne, const int4 *tetv, int tstride, const int4 *adja,
                                                         int astride, const int *part, int ncolor, int *P, int *flags) {
  int bad = 0;
  const int stride = (int)gridDim.x * kPBlock;
  for (int k = (int)blockIdx.x * kPBlock + (int)threadIdx.x; k < ne; k += stride) {
    if (tetv && tetv[(size_t)k * tstride].x <= 0) {
      P[k] = -1;
      bad |= MESH_UNUSED;
      continue;
    }
    const int c = part ? part[k] : 0;
    if ((unsigned int)c >= (unsigned int)ncolor) bad |= C_BADPART;
    const int4 a = adja[(size_t)k * astride];
    const int lk[4] = {a.x, a.y, a.z, a.w};
    int lo = k;
#pragma unroll
    for (int f = 0; f < 4; f++) {
      if (!lk[f]) continue;
      if (!link_ok(lk[f], ne)) {
        bad |= MESH_BADLINK;
        continue;
      }
      const int nb = lk[f] / 4 - 1;
      if (nb < lo && (!part || part[nb] == c)) lo = nb;
    }
    P[k] = lo;
  }
  if (bad) atomicOr(flags, bad);
}

// One hooking round on a flat forest: L[k] = P[k] = k's root.  L is only read; the hooks go to P, at roots, whose
// P word holds the root itself until then.  *changed: a plain store of 1 by whoever hooked.
__global__ __launch_bounds__(kPBlock) void k_contig_hook(int ne, const int4 *adja, int astride, const int *part,
                                                         const int *L, int *P, int *changed) {
  bool ch = false;
  const int stride = (int)gridDim.x * kPBlock;
  for (int k = (int)blockIdx.x * kPBlock + (int)threadIdx.x; k < ne; k += stride) {
    const int lk = L[k];
    if (lk < 0) continue;
    const int c = part ? part[k] : 0;
    const int4 a = adja[(size_t)k * astride];
    const int ln[4] = {a.x, a.y, a.z, a.w};
#pragma unroll
    for (int f = 0; f < 4; f++) {
      if (!ln[f]) continue;
      const int nb = ln[f] / 4 - 1;
      if (part && part[nb] != c) continue;
      const int lj = L[nb];
      if (lj == lk) continue;
      const int hi = lk > lj ? lk : lj, lo = lk > lj ? lj : lk;
      (void)__hip_atomic_fetch_min(&P[hi], lo, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      ch = true;
    }
  }
  if (ch) *changed = 1;
}

// One flatten pass on P: every tetra follows up to `jumps` parents, points at where it got to and notes it in L.
// A root's own word is not written by this kernel, so a chase that met one has met the final one, and a pass in
// which every chase did has left L[k] = P[k] = the root.  *unfinished: a plain store of 1 by a tetra whose chase
// stopped at the bound.
__global__ __launch_bounds__(kPBlock) void k_contig_flatten(int ne, int jumps, int *P, int *L, int *unfinished) {
  bool left = false;
  const int stride = (int)gridDim.x * kPBlock;
  for (int k = (int)blockIdx.x * kPBlock + (int)threadIdx.x; k < ne; k += stride) {
    const int p = P[k];
    int r = p;
    if (p >= 0 && p != k) {
      bool done = false;
      for (int i = 0; i < jumps; i++) {
        const int g = P[r];
        if (g == r) {
          done = true;
          break;
        }
        r = g;
      }
      if (r != p) P[k] = r;
      if (!done) left = true;
    }
    L[k] = r;
  }
  if (left) *unfinished = 1;
}

// heads (L[k] == k) of block b = tetra 256 b .. 256 b + 255
__global__ __launch_bounds__(kPBlock) void k_contig_heads_count(int ne, const int *L, int *btot) {
  __shared__ int wt[kPWaves];
  const int k = (int)blockIdx.x * kPBlock + (int)threadIdx.x;
  const int c = (k < ne && L[k] == k) ? 1 : 0;
  const int n = block_reduce<kPWaves>(c, wt, IntSum());
  if (threadIdx.x == 0) btot[blockIdx.x] = n;
}

// a head's row in the table (ascending head) and the row's start values
__global__ __launch_bounds__(kPBlock) void k_contig_heads_fill(int ne, const int *L, const int *part, const int *boff,
                                                               int *idx, ContigSub *sub) {
  __shared__ int wt[kPWaves];
  const int k = (int)blockIdx.x * kPBlock + (int)threadIdx.x;
  const bool head = k < ne && L[k] == k;
  int n;
  const int pos = boff[blockIdx.x] + block_prefix<kPWaves>(head ? 1 : 0, wt, &n);
  if (head) {
    idx[k] = pos;
    sub[pos] = ContigSub{part ? part[k] : 0, k + 1, 0, INT_MAX};
  }
}

// Sizes and exits of the rows.  A tetra's candidate is its lowest face towards another colour, 4 (k+1) + f.
__global__ __launch_bounds__(kPBlock) void k_contig_stats(int ne, const int4 *adja, int astride, const int *part,
                                                          const int *L, const int *idx, ContigSub *sub) {
  __shared__ SizeTable sizes;
  const auto size_of = [sub](int t) { return &sub[t].size; };
  sizes.clear<kPBlock>();
  __syncthreads();
  const int stride = (int)gridDim.x * kPBlock;
  const int lane = threadIdx.x & 63;
  for (int k0 = (int)blockIdx.x * kPBlock; k0 < ne; k0 += stride) { // (block-uniform: every lane is here)
    const int k = k0 + (int)threadIdx.x;
    const int l = k < ne ? L[k] : -1;
    const int t = l >= 0 ? idx[l] : -1;
    int cand = INT_MAX;
    if (t >= 0 && part) {
      const int c = part[k];
      const int4 a = adja[(size_t)k * astride];
      const int ln[4] = {a.x, a.y, a.z, a.w};
#pragma unroll
      for (int f = 3; f >= 0; f--)
        if (ln[f] && part[ln[f] / 4 - 1] != c) cand = 4 * (k + 1) + f;
    }
    const int t0 = __builtin_amdgcn_readfirstlane(t);
    if (__all(t == t0)) { // the wave's 64 tetra are in one row (or all beyond ne / unused)
      if (t0 >= 0) {
        for (int o = 32; o > 0; o >>= 1) {
          const int y = __shfl_down(cand, o);
          cand = y < cand ? y : cand;
        }
        if (lane == 0) {
          sizes.add(t0, 64, size_of);
          if (cand != INT_MAX) atomic_lower(&sub[t0].exit, cand);
        }
      }
    } else if (t >= 0) {
      sizes.add(t, 1, size_of);
      if (cand != INT_MAX) atomic_lower(&sub[t].exit, cand);
    }
  }
  __syncthreads();
  sizes.flush<kPBlock>(size_of);
}

// exit INT_MAX -> 0 (the row touches no other colour); else the colour across it
__global__ __launch_bounds__(kPBlock) void k_contig_exits(int nsub, const int *adja, int astride, const int *part,
                                                          ContigSub *sub, int *exitcol) {
  const int i = (int)blockIdx.x * kPBlock + (int)threadIdx.x;
  if (i >= nsub) return;
  const int e = sub[i].exit;
  if (e == INT_MAX) {
    sub[i].exit = 0;
    exitcol[i] = -1;
    return;
  }
  const int lk = adja[4 * (size_t)(e / 4 - 1) * astride + (e & 3)];
  exitcol[i] = part[lk / 4 - 1];
}

// head[k] = the subgroup's lowest tetra (1-based), flag[k] = rank[its row]; 0 for an unused tetra
__global__ __launch_bounds__(kPBlock) void k_contig_write(int ne, const int *L, const int *idx, const int *rank,
                                                          int *head, int *flag) {
  const int stride = (int)gridDim.x * kPBlock;
  for (int k = (int)blockIdx.x * kPBlock + (int)threadIdx.x; k < ne; k += stride) {
    const int l = L[k];
    if (head) head[k] = l + 1;
    if (flag) flag[k] = l >= 0 ? rank[idx[l]] : 0;
  }
}

// part[k] = target[its row] where that is a colour (>= 0)
__global__ __launch_bounds__(kPBlock) void k_contig_apply(int ne, const int *L, const int *idx, const int *target,
                                                          int *part) {
  const int stride = (int)gridDim.x * kPBlock;
  for (int k = (int)blockIdx.x * kPBlock + (int)threadIdx.x; k < ne; k += stride) {
    const int l = L[k];
    if (l < 0) continue;
    const int t = target[idx[l]];
    if (t >= 0) part[k] = t;
  }
}

// the largest vertex id of the tetra (np of a call that builds its adjacency): one atomic per block
__global__ __launch_bounds__(kPBlock) void k_contig_vmax(int ne, const int4 *tetv, int *vmax) {
  __shared__ int wt[kPWaves];
  int m = 0;
  const int stride = (int)gridDim.x * kPBlock;
  for (int k = (int)blockIdx.x * kPBlock + (int)threadIdx.x; k < ne; k += stride) {
    const int4 v = tetv[k];
    m = max(max(m, max(v.x, v.y)), max(v.z, v.w));
  }
  m = block_reduce<kPWaves>(m, wt, IntMax());
  if (threadIdx.x == 0) atomicMax(vmax, m);
}

int ceil_log2(int n) {
  int b = 0;
  while (b < 31 && (1LL << b) < n) b++;
  return b;
}

// the link rows of a call that came without any, built into the cache; np = the largest vertex id
int ensure_adja(hipStream_t s, TetView *m, ContigCache *c, SnapCache *snap, char *msg, size_t msglen) {
  if (m->adja || m->ne == 0) return 1;
  int *words = get<int>(c->words, W_COUNT);
  if (!words) {
    snprintf(msg, msglen, "contiguity: out of device memory (adjacency of %d tetra)", m->ne);
    return 0;
  }
  DEVCK(hipMemsetAsync(words, 0, W_COUNT * sizeof(int), s));
  hipLaunchKernelGGL(k_contig_vmax, dim3(grid_for(m->ne)), dim3(kPBlock), 0, s, m->ne, rows_of(*m).tetv,
                     words + W_VMAX);
  DEVCK(hipGetLastError());
  int np = 0;
  if (!read_word(s, words + W_VMAX, &np, msg, msglen)) return 0;
  if (np < 1) {
    snprintf(msg, msglen, "build_adjacency: vertex ids out of [1, np] or repeated in a tetra");
    return 0;
  }
  return built_adjacency(s, "contiguity", np, m, c->adja, snap, msg, msglen);
}

// L of the current colours.  fresh: from singletons, with the call's refusals (the checks of k_contig_init);
// else from L and P of the last labelling, after whole subgroups of it took another colour: each still
// carries its own lowest tetra, a valid root in the colour it joined, and only the joins remain to be
// hooked.  *rounds: hooking rounds, the fused first one and the idle last one included.
int label(hipStream_t s, const TetView &m, const int *part, int ncolor, bool fresh, ContigCache *c, int *rounds,
          char *msg, size_t msglen) {
  const int ne = m.ne, grid = grid_for(ne);
  int *L = get<int>(c->label, (size_t)ne), *P = get<int>(c->parent, (size_t)ne), *words = get<int>(c->words, W_COUNT);
  if (!L || !P || !words) {
    snprintf(msg, msglen, "contiguity: out of device memory (labels of %d tetra)", ne);
    return 0;
  }
  const int4 *tv = rows_of(m).tetv, *av = rows_of(m).adja;
  if (fresh) {
    DEVCK(hipMemsetAsync(words, 0, W_COUNT * sizeof(int), s));
    hipLaunchKernelGGL(k_contig_init, dim3(grid), dim3(kPBlock), 0, s, ne, tv, m.tstride, av, m.astride, part, ncolor,
                       P, words + W_FLAGS);
    DEVCK(hipGetLastError());
    int f = 0;
    if (!read_word(s, words + W_FLAGS, &f, msg, msglen)) return 0;
    if (f & MESH_BADLINK) {
      snprintf(msg, msglen, "contiguity: an adja entry lies outside [4, 4*%d+3] (nothing written)", ne);
      return 0;
    }
    if (f & C_BADPART) {
      snprintf(msg, msglen, "contiguity: a used tetra has a part value outside [0, %d) (nothing written)", ncolor);
      return 0;
    }
    if (!check_links<kPBlock>(s, "contiguity", " (nothing written)", m, words + W_FLAGS, &f, msg, msglen)) return 0;
  }
  const int cap = 2 * ceil_log2(ne > 2 ? ne : 2) + 1; // of the hooking rounds: the bound of the file's header
  const int pass_cap = ceil_log2(ne) + 2;             // of a round's flatten passes (17-fold each: ceil(log17 ne) + 1)
  int nround = fresh ? 1 : 0;
  bool flat = !fresh; // (the last labelling left every tetra at its root)
  for (;;) {
    for (int pass = 0; !flat; pass++) {
      if (pass == pass_cap) {
        snprintf(msg, msglen, "contiguity: the labels are not flat after %d passes (ne=%d)", pass_cap, ne);
        return 0;
      }
      DEVCK(hipMemsetAsync(words + W_PASS, 0, sizeof(int), s));
      hipLaunchKernelGGL(k_contig_flatten, dim3(grid), dim3(kPBlock), 0, s, ne, kCJumps, P, L, words + W_PASS);
      DEVCK(hipGetLastError());
      c->passes++;
      int left = 0;
      if (!read_word(s, words + W_PASS, &left, msg, msglen)) return 0;
      flat = !left;
    }
    if (nround == cap) {
      snprintf(msg, msglen, "contiguity: more than %d hooking rounds (ne=%d; is the adjacency symmetric?)", cap, ne);
      return 0;
    }
    DEVCK(hipMemsetAsync(words + W_PASS, 0, sizeof(int), s));
    hipLaunchKernelGGL(k_contig_hook, dim3(grid), dim3(kPBlock), 0, s, ne, av, m.astride, part, L, P, words + W_PASS);
    DEVCK(hipGetLastError());
    nround++;
    int changed = 0;
    if (!read_word(s, words + W_PASS, &changed, msg, msglen)) return 0;
    if (!changed) break;
    flat = false;
  }
  if (rounds) *rounds = nround;
  return 1;
}

// the table of the labelled forest, on the device (cache->sub, ->exitcol, ->idx) and on the host
int table(hipStream_t s, const TetView &m, const int *part, ContigCache *c, std::vector<ContigSub> *T,
          std::vector<int> *exitcol, char *msg, size_t msglen) {
  const int ne = m.ne, nblk = (ne + kPBlock - 1) / kPBlock;
  const int *L = c->label.as<int>();
  char oom[96];
  snprintf(oom, sizeof(oom), "contiguity: out of device memory (table index of %d tetra)", ne);
  int *idx = get<int>(c->idx, (size_t)ne);
  if (!idx) return refuse(msg, msglen, oom);
  if (!reserve(c->heads, nblk, s, oom, msg, msglen)) return 0;
  const int *boff = c->heads.boff.as<int>();
  hipLaunchKernelGGL(k_contig_heads_count, dim3(nblk), dim3(kPBlock), 0, s, ne, L, c->heads.btot.as<int>());
  DEVCK(hipGetLastError());
  int nsub = 0;
  if (!offsets(c->heads, s, nblk, &nsub, msg, msglen)) return 0;
  T->assign((size_t)nsub, ContigSub{0, 0, 0, 0});
  exitcol->assign((size_t)nsub, -1);
  if (nsub == 0) return 1;
  ContigSub *sub = get<ContigSub>(c->sub, (size_t)nsub);
  int *ec = get<int>(c->exitcol, (size_t)nsub);
  if (!sub || !ec || !get<int>(c->rank, (size_t)nsub)) {
    snprintf(msg, msglen, "contiguity: out of device memory (table of %d subgroups)", nsub);
    return 0;
  }
  const int4 *av = rows_of(m).adja;
  hipLaunchKernelGGL(k_contig_heads_fill, dim3(nblk), dim3(kPBlock), 0, s, ne, L, part, boff, idx, sub);
  hipLaunchKernelGGL(k_contig_stats, dim3(grid_for(ne)), dim3(kPBlock), 0, s, ne, av, m.astride, part, L, idx, sub);
  hipLaunchKernelGGL(k_contig_exits, dim3((nsub + kPBlock - 1) / kPBlock), dim3(kPBlock), 0, s, nsub, m.adja,
                     m.astride, part, sub, ec);
  DEVCK(hipGetLastError());
  DEVCK(hipMemcpyAsync(T->data(), sub, sizeof(ContigSub) * (size_t)nsub, hipMemcpyDeviceToHost, s));
  DEVCK(hipMemcpyAsync(exitcol->data(), ec, sizeof(int) * (size_t)nsub, hipMemcpyDeviceToHost, s));
  DEVCK(hipStreamSynchronize(s));
  return 1;
}

void count_colours(const std::vector<ContigSub> &T, int ncolor, int *ncomp) {
  for (int c = 0; c < ncolor; c++) ncomp[c] = 0;
  for (const ContigSub &r : T) ncomp[r.color]++;
}

} // namespace

int pmmg_contig_subgroups(hipStream_t s, TetView m, const int *part, int ncolor, int *head, int *flag, int *ncomp,
                          int cap, pmmg_hip_subgroup *sub, int64_t *nsub, int *rounds, ContigCache *cache,
                          SnapCache *snap, char *msg, size_t msglen) {
  *nsub = 0;
  cache->passes = 0;
  for (int c = 0; c < ncolor; c++) ncomp[c] = 0;
  if (rounds) *rounds = 0;
  if (m.ne == 0) return 1;
  if (!ensure_adja(s, &m, cache, snap, msg, msglen)) return 0;
  if (!label(s, m, part, ncolor, true, cache, rounds, msg, msglen)) return 0;
  std::vector<ContigSub> T;
  std::vector<int> exitcol;
  if (!table(s, m, part, cache, &T, &exitcol, msg, msglen)) return 0;
  *nsub = (int64_t)T.size();
  count_colours(T, ncolor, ncomp);
  if (head || flag) {
    // flag = 1 + the subgroups of the same colour with a lower head: finished here from the table (ascending head)
    std::vector<int> seen((size_t)ncolor, 0), rank(T.size());
    for (size_t i = 0; i < T.size(); i++) rank[i] = ++seen[(size_t)T[i].color];
    int *d_rank = cache->rank.as<int>();
    if (!T.empty()) DEVCK(hipMemcpyAsync(d_rank, rank.data(), sizeof(int) * rank.size(), hipMemcpyHostToDevice, s));
    hipLaunchKernelGGL(k_contig_write, dim3(grid_for(m.ne)), dim3(kPBlock), 0, s, m.ne, cache->label.as<int>(),
                       cache->idx.as<int>(), d_rank, head, flag);
    DEVCK(hipGetLastError());
    DEVCK(hipStreamSynchronize(s)); // (rank is read by the copy until here)
  }
  if ((int64_t)T.size() > (int64_t)cap) {
    snprintf(msg, msglen, "part_subgroups: %lld subgroups exceed cap = %d (nothing written to sub)",
             (long long)T.size(), cap);
    return 0;
  }
  for (size_t i = 0; i < T.size(); i++) {
    sub[i].color = T[i].color;
    sub[i].head = T[i].head;
    sub[i].size = T[i].size;
    sub[i].exit = T[i].exit;
  }
  return 1;
}

int pmmg_contig_fix(hipStream_t s, TetView m, int *part, int ncolor, int64_t *nmoved, int *nmerged, int *nstuck,
                    ContigCache *cache, SnapCache *snap, char *msg, size_t msglen) {
  *nmoved = 0;
  *nmerged = *nstuck = 0;
  cache->passes = 0;
  if (m.ne == 0) return 1;
  if (!ensure_adja(s, &m, cache, snap, msg, msglen)) return 0;
  if (!label(s, m, part, ncolor, true, cache, nullptr, msg, msglen)) return 0;
  std::vector<ContigSub> T;
  std::vector<int> exitcol, ncomp((size_t)ncolor, 0), target;
  if (!table(s, m, part, cache, &T, &exitcol, msg, msglen)) return 0;
  count_colours(T, ncolor, ncomp.data());
  bool any = false;
  for (int c = 0; c < ncolor; c++) any = any || ncomp[(size_t)c] > 1;
  if (!any) return 1; // the common case: every colour is one subgroup
  // Colour by colour.  A colour's rows are those of the last labelling as long as nothing was moved into it
  // since; the colours across its exits as long as nothing was moved at all.
  std::vector<char> dirty((size_t)ncolor, 0);
  bool stale = false;
  ContigCounts n;
  for (int c = 0; c < ncolor; c++) {
    if (dirty[(size_t)c] || (stale && ncomp[(size_t)c] > 1)) {
      if (!label(s, m, part, ncolor, false, cache, nullptr, msg, msglen)) return 0;
      if (!table(s, m, part, cache, &T, &exitcol, msg, msglen)) return 0;
      count_colours(T, ncolor, ncomp.data());
      dirty.assign((size_t)ncolor, 0);
      stale = false;
    }
    if (ncomp[(size_t)c] <= 1) continue;
    target.resize(T.size());
    if (!contig_decide(T.data(), exitcol.data(), (int64_t)T.size(), c, target.data(), &n)) continue;
    for (int t : target)
      if (t >= 0) dirty[(size_t)t] = 1;
    stale = true;
    int *d_target = cache->rank.as<int>();
    DEVCK(hipMemcpyAsync(d_target, target.data(), sizeof(int) * target.size(), hipMemcpyHostToDevice, s));
    hipLaunchKernelGGL(k_contig_apply, dim3(grid_for(m.ne)), dim3(kPBlock), 0, s, m.ne, cache->label.as<int>(),
                       cache->idx.as<int>(), d_target, part);
    DEVCK(hipGetLastError());
    DEVCK(hipStreamSynchronize(s));
  }
  *nmoved = n.nmoved;
  *nmerged = n.nmerged;
  *nstuck = n.nstuck;
  return 1;
}
