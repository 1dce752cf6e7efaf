// pmmg_meshstats.hip — the two reports ParMmg prints on an adapted mesh,
// reduced on the device from arrays that are already there.
//
// PMMG_qualhisto (reference src/quality_pmmg.c:156-345, called at
// src/libparmmg1.c:910) runs Mmg's MMG3D_computeOutqua per group: best,
// average and worst quality, the worst element, the counts above 0.12 and
// 0.5 and a 5-bin histogram.  PMMG_prilen / PMMG_computePrilen (:591-715,
// :370-574) hash every edge of the group (MMG5_hashEdge), pop each one once
// in ascending tetra order (MMG5_hashPop) and report its length in the
// metric: average, extremes with their end points, null edges and a 9-bin
// histogram.  Mmg @889d408 is not in the image: MMG3D_computeOutqua and the
// hash's pop order are restated from its published source (parity unpinned,
// like the rest of the Mmg boundary).  Not modelled: the
// ridge-point count nrid (needs Mmg's point tags), the metric storage at
// ridge points and the MG_GEO point filter of :510-517.
//
// The edge report needs the set of unique edges with one owner each.  An
// open-addressing table of 64-bit keys (min << 32 | max) with a parallel
// 32-bit owner code 6 k + ia, lowered by atomicMin, gives every edge the
// owner the reference's ascending loop gives it, whatever order the lanes
// run in.  One lane per tetra throughout.  Sums go through per-block
// partials in a slab that one block adds in a fixed order, so two calls on
// the same inputs return the same bytes.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>
#include <stdio.h>

#include "pmmg_meshstats.hpp"
#include "pmmg_devutil.hpp"
#include "pmmg_quality.hpp"

namespace {

constexpr int kSBlock = 256;
constexpr int kSWaves = kSBlock / 64;
constexpr int kMaxGrid = 8 * 256 * 8;          // grid-stride beyond 16K blocks (as pmmg_qual_tetra)
constexpr double kAlphaD = 20.7846096908265;   // MMG3D_ALPHAD = 12 sqrt(3)
constexpr unsigned long long kEmptyKey = ~0ULL;
constexpr unsigned long long kForeign = 1ULL << 63; // key bit of an edge from the skip list (ids are < 2^31)
constexpr unsigned int kNone = 0xffffffffu;         // no owner / no slot / no element
constexpr unsigned int kProbeLimit = 2048;          // probes before a table below its final size counts as full

__constant__ int kSIare[6][2] = {{0, 1}, {0, 2}, {0, 3}, {1, 2}, {1, 3}, {2, 3}}; // MMG5_iare
__constant__ double kBd[9] = {0.0, 0.3, 0.6, 0.7071, 0.9, 1.3, 1.4142, 2.0, 5.0};  // quality_pmmg.c:387

// ---------------------------------------------------------------- block reductions (fixed order)

__device__ __forceinline__ double wave_sum(double v) {
  for (int o = 32; o > 0; o >>= 1) v += __shfl_down(v, o);
  return v; // lane 0
}

// lexicographic minimum of (value, code): the smaller value, on equal values the smaller code
__device__ __forceinline__ void wave_min(double &v, unsigned int &c) {
  for (int o = 32; o > 0; o >>= 1) {
    const double ov = __shfl_down(v, o);
    const unsigned int oc = __shfl_down(c, o);
    if (ov < v || (ov == v && oc < c)) { v = ov; c = oc; }
  }
}

// the larger value, on equal values the smaller code
__device__ __forceinline__ void wave_max(double &v, unsigned int &c) {
  for (int o = 32; o > 0; o >>= 1) {
    const double ov = __shfl_down(v, o);
    const unsigned int oc = __shfl_down(c, o);
    if (ov > v || (ov == v && oc < c)) { v = ov; c = oc; }
  }
}

// one block's (or, in the final kernels, one thread's) partial: sum, extremes and their codes
struct Part {
  double sum, mn, mx;
  unsigned int cmn, cmx;
};

// reduces the threads' partials to one in thread 0 (waves combined in wave order)
__device__ __forceinline__ Part block_part(Part p) {
  __shared__ Part wp[kSWaves];
  p.sum = wave_sum(p.sum);
  wave_min(p.mn, p.cmn);
  wave_max(p.mx, p.cmx);
  if ((threadIdx.x & 63) == 0) wp[threadIdx.x >> 6] = p;
  __syncthreads();
  if (threadIdx.x == 0) {
    for (int w = 1; w < kSWaves; w++) {
      const Part q = wp[w];
      p.sum += q.sum;
      if (q.mn < p.mn || (q.mn == p.mn && q.cmn < p.cmn)) { p.mn = q.mn; p.cmn = q.cmn; }
      if (q.mx > p.mx || (q.mx == p.mx && q.cmx < p.cmx)) { p.mx = q.mx; p.cmx = q.cmx; }
    }
  }
  return p;
}

// the slab's nblk partials into one, by one block: thread t takes blocks t, t + 256, ... in ascending
// order, then the threads are combined as above
__device__ __forceinline__ Part slab_part(const Part *slab, int nblk, double mn0, double mx0) {
  Part p{0.0, mn0, mx0, kNone, kNone};
  for (int b = threadIdx.x; b < nblk; b += kSBlock) {
    const Part q = slab[b];
    p.sum += q.sum;
    if (q.mn < p.mn || (q.mn == p.mn && q.cmn < p.cmn)) { p.mn = q.mn; p.cmn = q.cmn; }
    if (q.mx > p.mx || (q.mx == p.mx && q.cmx < p.cmx)) { p.mx = q.mx; p.cmx = q.cmx; }
  }
  return block_part(p);
}

// ---------------------------------------------------------------- quality histogram

enum { Q_USED, Q_GOOD, Q_MED, Q_HIS0, Q_COUNT = Q_HIS0 + 5 };

// MMG3D_computeOutqua over the used tetra: counts and bins through LDS and one integer atomic per
// counter and block, sum / max / (min, row) as the block's partial
__global__ __launch_bounds__(kSBlock) void k_qual_histo(int ne, const int4 *tetv, const double *qual, Part *slab,
                                                        unsigned long long *cnt) {
  __shared__ unsigned int sh[Q_COUNT];
  if (threadIdx.x < Q_COUNT) sh[threadIdx.x] = 0;
  __syncthreads();
  Part p{0.0, 2.0, 0.0, kNone, kNone};
  const int stride = gridDim.x * blockDim.x;
  for (int k = blockIdx.x * blockDim.x + threadIdx.x; k < ne; k += stride) {
    if (tetv[k].x <= 0) continue;
    const double rap = kAlphaD * qual[k];
    atomicAdd(&sh[Q_USED], 1u);
    if (rap < p.mn) { p.mn = rap; p.cmn = (unsigned int)k; } // (ascending k: the lowest row on equal minima)
    if (rap > p.mx) { p.mx = rap; p.cmx = (unsigned int)k; }
    p.sum += rap;
    if (rap > 0.12) atomicAdd(&sh[Q_GOOD], 1u);
    if (rap > 0.5) atomicAdd(&sh[Q_MED], 1u);
    int ir = (int)(5.0 * rap);
    ir = ir > 4 ? 4 : (ir < 0 ? 0 : ir); // (a quality is never negative; the bin index stays in range for any input)
    atomicAdd(&sh[Q_HIS0 + ir], 1u);
  }
  p = block_part(p);
  if (threadIdx.x == 0) slab[blockIdx.x] = p;
  __syncthreads();
  if (threadIdx.x < Q_COUNT && sh[threadIdx.x]) atomicAdd(&cnt[threadIdx.x], (unsigned long long)sh[threadIdx.x]);
}

__global__ __launch_bounds__(kSBlock) void k_qual_final(const Part *slab, int nblk, const unsigned long long *cnt,
                                                        pmmg_hip_qual_histo_t *out) {
  const Part p = slab_part(slab, nblk, 2.0, 0.0);
  if (threadIdx.x != 0) return;
  pmmg_hip_qual_histo_t r{};
  r.ne_used = (int64_t)cnt[Q_USED];
  r.max = p.mx;
  r.min = p.mn;
  r.iel = p.cmn == kNone ? 0 : (int64_t)p.cmn + 1;
  r.avg_sum = p.sum;
  r.good = (int64_t)cnt[Q_GOOD];
  r.med = (int64_t)cnt[Q_MED];
  for (int i = 0; i < 5; i++) r.his[i] = (int64_t)cnt[Q_HIS0 + i];
  *out = r;
}

// ---------------------------------------------------------------- edge table

struct Table {
  unsigned long long *keys; // kEmptyKey, or min << 32 | max (| kForeign)
  unsigned int *own;        // lowest 6 k + ia that inserted the key (kNone: a skip pair that is no mesh edge)
  unsigned int nslot;
  unsigned int limit;       // probes before giving up (at the final size the whole table: cannot fail)
  unsigned int per;         // hash mode 1: slots per low vertex (0: mode 0, see probe_first)
};

__device__ __forceinline__ unsigned long long mix64(unsigned int mn, unsigned int mx) {
  unsigned long long h = ((unsigned long long)mn << 32) | mx; // (murmur3's finaliser)
  h ^= h >> 33;
  h *= 0xff51afd7ed558ccdULL;
  h ^= h >> 33;
  h *= 0xc4ceb9fe1a85ec53ULL;
  h ^= h >> 33;
  return h;
}

// The probe sequence of a key.  Mode 0 (per == 0): linear from a mix of the whole key; it visits every
// slot, so at the table's final size an insertion cannot fail.  Mode 1: the first kLocalProbes slots are
// linear from a run of `per` slots per low vertex (the other end picks one of its first 8), so the edges
// of one low vertex stay within two or three neighbouring lines and those of neighbouring vertices in
// neighbouring runs, which a spatially coherent numbering keeps in L2; a key that finds its run crowded (a
// vertex of high degree, a badly spread numbering) goes on from the mix of the key in steps of a second
// mix of it (linear steps from there would run through the stretches the local probes fill: CPU model of a
// shuffled 14K-vertex shell, longest sequence 151 probes against 32).
constexpr unsigned int kLocalProbes = 16;

struct Probe {
  unsigned int s, step;
};

__device__ __forceinline__ Probe probe_first(const Table &T, unsigned int mn, unsigned int mx) {
  Probe p;
  p.step = 1u;
  if (T.per) {
    p.s = (mn - 1u) * T.per + ((mx * 0x9E3779B1u) >> 29);
    if (p.s >= T.nslot) p.s %= T.nslot;
  } else {
    p.s = (unsigned int)(((mix64(mn, mx) >> 32) * (unsigned long long)T.nslot) >> 32);
  }
  return p;
}

// moves to the next slot, n probes having been made
__device__ __forceinline__ void probe_next(const Table &T, Probe &p, unsigned int n, unsigned int mn,
                                           unsigned int mx) {
  if (T.per && n == kLocalProbes) {
    const unsigned long long h = mix64(mn, mx);
    p.s = (unsigned int)(((h >> 32) * (unsigned long long)T.nslot) >> 32);
    p.step = 1u + (unsigned int)(((h & 0xffffffffULL) * (unsigned long long)(T.nslot - 1u)) >> 32); // 1 .. nslot - 1
    return;
  }
  p.s = p.step >= T.nslot - p.s ? p.s - (T.nslot - p.step) : p.s + p.step;
}

// the slot of key (with or without kForeign), kNone when it is absent
__device__ __forceinline__ unsigned int tab_find(const Table &T, unsigned int mn, unsigned int mx) {
  const unsigned long long key = ((unsigned long long)mn << 32) | mx;
  Probe p = probe_first(T, mn, mx);
  for (unsigned int n = 0; n < T.limit; n++) {
    const unsigned long long cur = T.keys[p.s];
    if ((cur & ~kForeign) == key) return p.s;
    if (cur == kEmptyKey) return kNone;
    probe_next(T, p, n + 1, mn, mx);
  }
  return kNone;
}

enum { F_FULL = 0, F_BADID = 1 };

// the skip list first: keys marked foreign, no owner.  Pairs outside [1, np] or with equal ends cannot be
// mesh edges and are dropped here; repeats and both orientations meet in one slot.
__global__ __launch_bounds__(kSBlock) void k_edge_skip(Table T, int np, int nskip, const int2 *skip, int *flags) {
  for (int j = blockIdx.x * blockDim.x + threadIdx.x; j < nskip; j += gridDim.x * blockDim.x) {
    const int2 e = skip[j];
    if (e.x < 1 || e.y < 1 || e.x > np || e.y > np || e.x == e.y) continue;
    const unsigned int mn = e.x < e.y ? e.x : e.y, mx = e.x < e.y ? e.y : e.x;
    const unsigned long long key = (((unsigned long long)mn << 32) | mx) | kForeign;
    Probe p = probe_first(T, mn, mx);
    bool done = false;
    for (unsigned int n = 0; n < T.limit && !done; n++) {
      unsigned long long cur = T.keys[p.s];
      if (cur == kEmptyKey) {
        cur = atomicCAS(&T.keys[p.s], kEmptyKey, key);
        if (cur == kEmptyKey) cur = key;
      }
      done = cur == key;
      if (!done) probe_next(T, p, n + 1, mn, mx);
    }
    if (!done) atomicOr(&flags[F_FULL], 1);
  }
}

// own pass: every used tetra inserts its 6 keys and lowers the slot's owner code to 6 k + ia.  A slot
// goes from empty to its key once and never changes again, so a plain load that sees a key sees the
// final one, and one that sees a stale empty is corrected by the CAS; an owner code only falls, so a
// plain load that is already <= the lane's code makes the atomicMin unnecessary.
__global__ __launch_bounds__(kSBlock) void k_edge_own(Table T, int np, int ne, const int4 *tetv, int *flags) {
  const int stride = gridDim.x * blockDim.x;
  for (int k = blockIdx.x * blockDim.x + threadIdx.x; k < ne; k += stride) {
    const int4 t = tetv[k];
    if (t.x <= 0) continue;
    const int v[4] = {t.x, t.y, t.z, t.w};
    if (t.x > np || t.y < 1 || t.y > np || t.z < 1 || t.z > np || t.w < 1 || t.w > np) {
      atomicOr(&flags[F_BADID], 1);
      continue;
    }
    for (int ia = 0; ia < 6; ia++) {
      const unsigned int a = v[kSIare[ia][0]], b = v[kSIare[ia][1]];
      const unsigned int mn = a < b ? a : b, mx = a < b ? b : a;
      const unsigned long long key = ((unsigned long long)mn << 32) | mx;
      const unsigned int code = 6u * (unsigned int)k + ia;
      Probe p = probe_first(T, mn, mx);
      bool done = false;
      for (unsigned int n = 0; n < T.limit && !done; n++) {
        unsigned long long cur = T.keys[p.s];
        if (cur == kEmptyKey) {
          cur = atomicCAS(&T.keys[p.s], kEmptyKey, key);
          if (cur == kEmptyKey) cur = key;
        }
        if ((cur & ~kForeign) == key) {
          if (T.own[p.s] > code) atomicMin(&T.own[p.s], code);
          done = true;
        } else {
          probe_next(T, p, n + 1, mn, mx);
        }
      }
      if (!done) atomicOr(&flags[F_FULL], 1);
    }
  }
}

__device__ __forceinline__ double edge_len(const double *xyz, int ani, const double *met, int ip1, int ip2) {
  const double *ca = xyz + 3 * (size_t)(ip1 - 1), *cb = xyz + 3 * (size_t)(ip2 - 1);
  return ani ? lenedg_ani(ca, cb, met + 6 * (size_t)(ip1 - 1), met + 6 * (size_t)(ip2 - 1))
             : lenedg_iso(ca, cb, met[ip1 - 1], met[ip2 - 1]);
}

enum { E_NEDGE, E_NSKIP, E_NED, E_NNULL, E_HL0, E_COUNT = E_HL0 + 9 };

// analyse pass (after k_edge_own has finished): each tetra looks its 6 edges up; where the owner code is
// its own it counts the edge and, unless the key is foreign, measures it (quality_pmmg.c:534-561).
// mask[k]: bit ia set for the edges tetra k analysed (the list pass reads it).
__global__ __launch_bounds__(kSBlock) void k_edge_analyse(Table T, const double *xyz, int ne, const int4 *tetv,
                                                          int ani, const double *met, unsigned char *mask,
                                                          Part *slab, unsigned long long *cnt) {
  __shared__ unsigned int sh[E_COUNT];
  if (threadIdx.x < E_COUNT) sh[threadIdx.x] = 0;
  __syncthreads();
  Part p{0.0, 1.e30, 0.0, kNone, kNone};
  const int stride = gridDim.x * blockDim.x;
  for (int k = blockIdx.x * blockDim.x + threadIdx.x; k < ne; k += stride) {
    const int4 t = tetv[k];
    unsigned int m = 0;
    if (t.x > 0) {
      const int v[4] = {t.x, t.y, t.z, t.w};
      for (int ia = 0; ia < 6; ia++) {
        const int np_ = v[kSIare[ia][0]], nq = v[kSIare[ia][1]];
        const unsigned int a = np_, b = nq;
        const unsigned int code = 6u * (unsigned int)k + ia;
        const unsigned int s = tab_find(T, a < b ? a : b, a < b ? b : a);
        if (s == kNone || T.own[s] != code) continue;
        atomicAdd(&sh[E_NEDGE], 1u);
        if (T.keys[s] & kForeign) {
          atomicAdd(&sh[E_NSKIP], 1u);
          continue;
        }
        m |= 1u << ia;
        const double len = edge_len(xyz, ani, met, np_, nq);
        if (!len) {
          atomicAdd(&sh[E_NNULL], 1u);
        } else {
          p.sum += len;
          atomicAdd(&sh[E_NED], 1u);
          if (len < p.mn) { p.mn = len; p.cmn = code; } // (ascending code within the lane: strict <)
          if (len > p.mx) { p.mx = len; p.cmx = code; }
          int i;
          for (i = 0; i < 8; i++)
            if (kBd[i] <= len && len < kBd[i + 1]) break;
          atomicAdd(&sh[E_HL0 + i], 1u);
        }
      }
    }
    mask[k] = (unsigned char)m;
  }
  p = block_part(p);
  if (threadIdx.x == 0) slab[blockIdx.x] = p;
  __syncthreads();
  if (threadIdx.x < E_COUNT && sh[threadIdx.x]) atomicAdd(&cnt[threadIdx.x], (unsigned long long)sh[threadIdx.x]);
}

__global__ __launch_bounds__(kSBlock) void k_edge_final(const Part *slab, int nblk, const unsigned long long *cnt,
                                                        const int4 *tetv, pmmg_hip_len_histo_t *out) {
  const Part p = slab_part(slab, nblk, 1.e30, 0.0);
  if (threadIdx.x != 0) return;
  pmmg_hip_len_histo_t r{};
  r.nedge = (int64_t)cnt[E_NEDGE];
  r.nskipped = (int64_t)cnt[E_NSKIP];
  r.ned = (int64_t)cnt[E_NED];
  r.nnull = (int64_t)cnt[E_NNULL];
  r.avlen_sum = p.sum;
  r.lmin = p.mn;
  r.lmax = p.mx;
  if (p.cmn != kNone) {
    const int4 t = tetv[p.cmn / 6u];
    const int v[4] = {t.x, t.y, t.z, t.w};
    r.amin = v[kSIare[p.cmn % 6u][0]];
    r.bmin = v[kSIare[p.cmn % 6u][1]];
  }
  if (p.cmx != kNone) {
    const int4 t = tetv[p.cmx / 6u];
    const int v[4] = {t.x, t.y, t.z, t.w};
    r.amax = v[kSIare[p.cmx % 6u][0]];
    r.bmax = v[kSIare[p.cmx % 6u][1]];
  }
  for (int i = 0; i < 9; i++) r.hl[i] = (int64_t)cnt[E_HL0 + i];
  *out = r;
}

// ---------------------------------------------------------------- list pass (block b = tetra 256 b ...)

__global__ __launch_bounds__(kSBlock) void k_list_count(int ne, const unsigned char *mask, int *btot) {
  __shared__ int wt[kSWaves];
  const long long k = (long long)blockIdx.x * kSBlock + threadIdx.x;
  const int n = block_reduce<kSWaves>(k < ne ? __popc((unsigned int)mask[k]) : 0, wt, IntSum());
  if (threadIdx.x == 0) btot[blockIdx.x] = n;
}

// boff[b]: analysed edges before block b.  Edge (k, ia) goes to row boff[b] + those before it in the
// block: ascending (owner tetra, ia).  cap >= the total (checked by the caller).
__global__ __launch_bounds__(kSBlock) void k_list_scatter(const double *xyz, int ne, const int4 *tetv, int ani,
                                                          const double *met, const unsigned char *mask,
                                                          const int *boff, int cap, int2 *edge_out, double *len_out) {
  __shared__ int wt[kSWaves];
  const long long k = (long long)blockIdx.x * kSBlock + threadIdx.x;
  const unsigned int m = k < ne ? mask[k] : 0u;
  int n;
  int pos = boff[blockIdx.x] + block_prefix<kSWaves>(__popc(m), wt, &n);
  if (!m) return;
  const int4 t = tetv[k];
  const int v[4] = {t.x, t.y, t.z, t.w};
  for (int ia = 0; ia < 6; ia++) {
    if (!(m & (1u << ia))) continue;
    const int np_ = v[kSIare[ia][0]], nq = v[kSIare[ia][1]];
    if (pos >= 0 && pos < cap) {
      if (edge_out) edge_out[pos] = make_int2(np_, nq);
      if (len_out) len_out[pos] = edge_len(xyz, ani, met, np_, nq);
    }
    pos++;
  }
}

// ---------------------------------------------------------------- host side

int grid_of(long long n) {
  const long long need = (n + kSBlock - 1) / kSBlock;
  return (int)(need < 1 ? 1 : (need < kMaxGrid ? need : kMaxGrid));
}

constexpr int kSmallCnt = 32; // StatsCache::small: 32 counters, then the 2 flags

} // namespace

int64_t pmmg_stats_cache_bytes(const StatsCache *c) {
  int64_t b = 0;
  if (c)
    for (const DevBuf *d : {&c->keys, &c->own, &c->small, &c->slab, &c->mask, &c->res, &c->list.btot, &c->list.boff, &c->list.tmp})
      b += (int64_t)d->cap;
  return b;
}

int pmmg_stats_qual_histo(hipStream_t s, int ne, const int *tetv, const double *qual, pmmg_hip_qual_histo_t *out,
                          StatsCache *cache, char *msg, size_t msglen) {
  const int nblk = grid_of(ne);
  unsigned long long *cnt = get<unsigned long long>(cache->small, kSmallCnt + 2);
  Part *slab = get<Part>(cache->slab, (size_t)kMaxGrid);
  pmmg_hip_qual_histo_t *res = reinterpret_cast<pmmg_hip_qual_histo_t *>(get<char>(cache->res, 512));
  if (!cnt || !slab || !res) {
    snprintf(msg, msglen, "qual_histo: out of device memory");
    return 0;
  }
  DEVCK(hipMemsetAsync(cnt, 0, sizeof(unsigned long long) * (kSmallCnt + 2), s));
  hipLaunchKernelGGL(k_qual_histo, dim3(nblk), dim3(kSBlock), 0, s, ne, reinterpret_cast<const int4 *>(tetv), qual,
                     slab, cnt);
  hipLaunchKernelGGL(k_qual_final, dim3(1), dim3(kSBlock), 0, s, slab, nblk, cnt, res);
  DEVCK(hipGetLastError());
  DEVCK(hipMemcpyAsync(out, res, sizeof(*out), hipMemcpyDeviceToHost, s));
  DEVCK(hipStreamSynchronize(s));
  return 1;
}

int pmmg_stats_edge_lengths(hipStream_t s, int np, const double *xyz, int ne, const int *tetv, int met_size,
                            const double *met, int nskip, const int *skip, pmmg_hip_len_histo_t *out, int cap,
                            int *edge_out, double *len_out, int hash_mode, StatsCache *cache, char *msg,
                            size_t msglen) {
  const int ani = met_size == 6 ? 1 : 0;
  const int4 *tv = reinterpret_cast<const int4 *>(tetv);
  if (6LL * ne > 0xfffffff0LL) {
    snprintf(msg, msglen, "edge_lengths: %d tetra exceed the 6*k+ia owner encoding (2^32)", ne);
    return 0;
  }
  // Table size.  A tetra mesh has close to 7 np edges (Mmg sizes its hash 7 np, quality_pmmg.c:422), so
  // 12 np + 2 nskip slots are about half full; never more than twice the keys that can be inserted,
  // 6 ne + nskip, at which size (load <= 1/2, whole-table probes) an insertion cannot fail.  Any tetv is
  // legal, so a table below that size that fills up (a probe limit, a device flag) is doubled and the
  // passes run again.
  const long long nkeys = 6LL * ne + nskip;
  const long long final_slots = 2 * nkeys > 64 ? 2 * nkeys : 64;
  long long nslot = 12LL * np + 2LL * nskip;
  if (nslot < 64) nslot = 64;
  if (nslot > final_slots) nslot = final_slots;
  if (cache->grown_np == np && cache->grown_ne == ne && cache->grown_nskip == nskip && cache->grown_mode == hash_mode &&
      cache->grown_nslot > nslot)
    nslot = cache->grown_nslot; // (the size the last call on a mesh of these counts had to grow to)
  const int nblk = grid_of(ne);
  unsigned long long *cnt = get<unsigned long long>(cache->small, kSmallCnt + 2);
  Part *slab = get<Part>(cache->slab, (size_t)kMaxGrid);
  unsigned char *mask = get<unsigned char>(cache->mask, (size_t)ne);
  pmmg_hip_len_histo_t *res = reinterpret_cast<pmmg_hip_len_histo_t *>(get<char>(cache->res, 512));
  if (!cnt || !slab || !mask || !res) {
    snprintf(msg, msglen, "edge_lengths: out of device memory");
    return 0;
  }
  int *flags = reinterpret_cast<int *>(cnt + kSmallCnt);
  Table T{};
  for (;;) {
    if (nslot > 0xfffffff0LL) {
      snprintf(msg, msglen, "edge_lengths: the edge table would exceed 2^32 slots");
      return 0;
    }
    T.keys = get<unsigned long long>(cache->keys, (size_t)nslot);
    T.own = get<unsigned int>(cache->own, (size_t)nslot);
    if (!T.keys || !T.own) {
      snprintf(msg, msglen, "edge_lengths: out of device memory (edge table of %lld slots)", nslot);
      return 0;
    }
    T.nslot = (unsigned int)nslot;
    T.limit = nslot >= final_slots ? T.nslot : (T.nslot < kProbeLimit ? T.nslot : kProbeLimit);
    T.per = 0; // (mode 1 below the final size only: its stepped sequence need not visit every slot)
    if (hash_mode == 1 && nslot < final_slots) T.per = nslot / np > 1 ? (unsigned int)(nslot / np) : 1u;
    DEVCK(hipMemsetAsync(T.keys, 0xff, sizeof(unsigned long long) * (size_t)nslot, s));
    DEVCK(hipMemsetAsync(T.own, 0xff, sizeof(unsigned int) * (size_t)nslot, s));
    DEVCK(hipMemsetAsync(cnt, 0, sizeof(unsigned long long) * (kSmallCnt + 2), s));
    if (nskip > 0)
      hipLaunchKernelGGL(k_edge_skip, dim3(grid_of(nskip)), dim3(kSBlock), 0, s, T, np, nskip,
                         reinterpret_cast<const int2 *>(skip), flags);
    hipLaunchKernelGGL(k_edge_own, dim3(nblk), dim3(kSBlock), 0, s, T, np, ne, tv, flags);
    DEVCK(hipGetLastError());
    int h_flags[2] = {0, 0};
    DEVCK(hipMemcpyAsync(h_flags, flags, sizeof(h_flags), hipMemcpyDeviceToHost, s));
    DEVCK(hipStreamSynchronize(s));
    if (h_flags[F_BADID]) {
      snprintf(msg, msglen, "edge_lengths: a used tetra has a vertex id outside [1, %d]", np);
      return 0;
    }
    if (!h_flags[F_FULL]) break;
    if (nslot >= final_slots) { // (cannot happen: whole-table probes at load <= 1/2)
      snprintf(msg, msglen, "edge_lengths: edge table of %lld slots full", nslot);
      return 0;
    }
    nslot = 2 * nslot < final_slots ? 2 * nslot : final_slots;
    cache->grown_np = np;
    cache->grown_ne = ne;
    cache->grown_nskip = nskip;
    cache->grown_mode = hash_mode;
    cache->grown_nslot = nslot;
  }
  hipLaunchKernelGGL(k_edge_analyse, dim3(nblk), dim3(kSBlock), 0, s, T, xyz, ne, tv, ani, met, mask, slab, cnt);
  hipLaunchKernelGGL(k_edge_final, dim3(1), dim3(kSBlock), 0, s, slab, nblk, cnt, tv, res);
  DEVCK(hipGetLastError());
  DEVCK(hipMemcpyAsync(out, res, sizeof(*out), hipMemcpyDeviceToHost, s));
  DEVCK(hipStreamSynchronize(s));
  if (!edge_out && !len_out) return 1;
  const long long nlist = (long long)(out->nedge - out->nskipped);
  if (nlist > cap) {
    snprintf(msg, msglen, "edge_lengths: %lld analysed edges exceed cap = %d (nothing written to the lists)", nlist,
             cap);
    return 0;
  }
  if (ne == 0) return 1;
  const int lblk = (ne + kSBlock - 1) / kSBlock;
  if (!reserve(cache->list, lblk, s, "edge_lengths: out of device memory (list pass)", msg, msglen)) return 0;
  hipLaunchKernelGGL(k_list_count, dim3(lblk), dim3(kSBlock), 0, s, ne, mask, cache->list.btot.as<int>());
  if (!offsets(cache->list, s, lblk, nullptr, msg, msglen)) return 0; // (the total is out->nedge - out->nskipped)
  hipLaunchKernelGGL(k_list_scatter, dim3(lblk), dim3(kSBlock), 0, s, xyz, ne, tv, ani, met, mask,
                     cache->list.boff.as<int>(), cap,
                     reinterpret_cast<int2 *>(edge_out), len_out);
  DEVCK(hipGetLastError());
  DEVCK(hipStreamSynchronize(s));
  return 1;
}
