// pmmg_fallback.hpp — exhaustive searches with the reference's semantics
// (included by pmmg_hip.hip only):
//   volume:  PMMG_locatePoint_exhaustTetra (locate_pmmg.c:737-770): the
//            lowest-index accepting tetra, else the closest tetra (argmin
//            |bary_min| * vol, :453-458) and its nearest vertex
//            (PMMG_barycoord3d_getClosest, barycoord_pmmg.c:371-404)
//   surface: PMMG_locatePoint_exhaustTria (locate_pmmg.c:477-515): the
//            lowest-index accepting tria, else the closest tria by centroid
//            distance with the stale re-evaluation of :505-509
// The query lists and their counts are produced on the device by the walks;
// every kernel here reads the count itself and returns at once when its list
// is empty, so the host launches them unconditionally (no read-back).
//
// Two launches per class (r05; r04's merged scan issued one contended global
// atomicMin per (element, query) pair and took a carried ParMmg iteration
// from 0.24 to 6.7 s), each one kernel template over the element kind (NV = 4
// tetra, 3 tria); what the classes differ in is FbElem<NV>:
//   accept   element-major: each thread holds one element and its bounding
//            box inflated past what the acceptance test can pass, and tests
//            the queries of the list in the grid cells the box covers (a
//            grid over the list built when the list is complete, k_fb_grid);
//            only the few pairs inside the box run the reference's test (one
//            atomicMin per accepting pair).  The last block interpolates the
//            accepted queries and lists the others.
//   closest  query-major, only for the queries nothing accepted (points
//            outside the domain): elements staged in LDS tiles, every lane
//            keeps its query's running (key, index) minimum over a range of
//            elements in index order (several lanes per query when the list
//            is short), the ranges' minima merged in the last block, which
//            interpolates.  No global atomics per pair.
#pragma once

#include "pmmg_prep.hpp"

namespace pmmg {

// The last block of a grid to get here returns true: the other blocks'
// results are then visible to it.  The barrier before the ticket: every wave
// of the block has issued its atomics (r04l: without it a block's later waves
// could still be scanning when the last block read the results — 4 surface
// points left unprocessed, once).  wrote: this thread stored data the last
// block reads; a block any of whose threads did releases it first
// (__threadfence).  The release is an L2 write-back on gfx950 (the XCDs' L2s
// are not coherent with each other): taken in every block of k_bdy (808
// blocks for a 205k-point group) it took the kernel 17 -> 87 us and slowed
// the volume kernel beside it (r05h trace) — only the blocks that wrote pay it.
__device__ __forceinline__ bool last_block(unsigned *done, bool wrote) {
  if (__syncthreads_or(wrote)) __threadfence();
  __shared__ bool last;
  if (threadIdx.x == 0) last = atomicAdd(done, 1u) == gridDim.x - 1;
  __syncthreads();
  if (last) __threadfence();
  return last;
}

__device__ __forceinline__ int load_agent(const int *p) {
  return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// The bounding box of an element inflated so that every point its
// acceptance test can pass lies inside.  Volume: every barycentric
// coordinate > -EPS puts x within 3 EPS of the extent outside the vertices'
// box (x_c = sum_i b_i p_ic, sum_i b_i = 1); the pad is 1e-4 of the extent
// (33x that, room for the coordinates' rounding on any element with an
// aspect ratio below ~1e10) plus 1e-12 of the coordinates' magnitude.
// Surface: the projection is inside the tria within the same margin and
// |dist| <= hausd along the unit normal.  A degenerate element (zero or
// non-finite volume / area) gets an infinite box: every query takes the
// reference's test there, as in the oracle.
constexpr double kBoxRel = 1e-4, kBoxAbs = 1e-12;
struct Box {
  double lo[3], hi[3];
};
__device__ __forceinline__ bool in_box(const Box &b, const double *x) {
  // NaN coordinates compare false everywhere and fall through to the test
  return !(x[0] < b.lo[0] || x[0] > b.hi[0] || x[1] < b.lo[1] || x[1] > b.hi[1] || x[2] < b.lo[2] ||
           x[2] > b.hi[2]);
}
template <int NV>
__device__ __forceinline__ Box elem_box(const double (*p)[3], double extra, bool degenerate) {
  Box b;
#pragma unroll
  for (int c = 0; c < 3; c++) {
    double lo = p[0][c], hi = p[0][c];
#pragma unroll
    for (int v = 1; v < NV; v++) {
      lo = fmin(lo, p[v][c]);
      hi = fmax(hi, p[v][c]);
    }
    const double pad = kBoxRel * (hi - lo) + kBoxAbs * fmax(fabs(lo), fabs(hi)) + extra + 1e-300;
    b.lo[c] = degenerate ? -INFINITY : lo - pad;
    b.hi[c] = degenerate ? INFINITY : hi + pad;
  }
  return b;
}

// ---------------------------------------------------------------- query grids
//
// The accept scans test an element only against the fallback queries in the
// grid cells its inflated box covers (r05: against every query of the list,
// the scan cost ne x nfb box tests — 92 ms for 2644 queries over 120M tetra
// in a carried iteration).  The grid is built by k_fb_grid, launched after
// the kernel that finishes the list (k_vol, k_bdy): G^3 cells over the
// queries' box, G = cbrt(nfb / 4) + 1 <= kFbGridMax; cells[c] .. cells[c + 1]
// index items[], the list positions of cell c's queries.  A query inside an
// element's box is in a cell of the box's (clamped) cell range, so the pairs
// tested are a superset of the accepting pairs: the same results as the full
// scan.
__device__ __forceinline__ int fb_cell1(double x, double lo, double inv, int G) {
  const double t = (x - lo) * inv;
  return t > 0.0 ? (t < (double)G ? (int)t : G - 1) : 0; // NaN -> 0, +inf -> G - 1
}

// one block: the grid of the list fb[0, nfb) into the class's state f;
// cells[kFbCells + 1] starts, cur[kFbCells] scratch, items[nfb]
__device__ __noinline__ void fb_grid_build(const double *qxyz, const int *fb, int nfb, FbState *f, int *cells,
                                           int *cur, int *items) {
  __shared__ double rlo[3][kBlock / 64], rhi[3][kBlock / 64]; // per-wave partial boxes
  __shared__ int sG;
  const int t = threadIdx.x, nt = blockDim.x, w = t >> 6, nw = (nt + 63) >> 6;
  double lo[3] = {INFINITY, INFINITY, INFINITY}, hi[3] = {-INFINITY, -INFINITY, -INFINITY};
  for (int j = t; j < nfb; j += nt) {
    double x[3];
    load_pt(qxyz, fb[j], x);
    for (int d = 0; d < 3; d++) {
      lo[d] = fmin(lo[d], x[d]);
      hi[d] = fmax(hi[d], x[d]);
    }
  }
  for (int d = 0; d < 3; d++)
    for (int o = 32; o > 0; o >>= 1) {
      lo[d] = fmin(lo[d], __shfl_xor(lo[d], o));
      hi[d] = fmax(hi[d], __shfl_xor(hi[d], o));
    }
  if (__lane_id() == 0)
    for (int d = 0; d < 3; d++) {
      rlo[d][w] = lo[d];
      rhi[d][w] = hi[d];
    }
  __syncthreads();
  if (t == 0) {
    for (int d = 0; d < 3; d++) {
      double a = INFINITY, b = -INFINITY;
      for (int i = 0; i < nw; i++) {
        a = fmin(a, rlo[d][i]);
        b = fmax(b, rhi[d][i]);
      }
      rlo[d][0] = a;
      rhi[d][0] = b;
    }
    int G = (int)cbrt((double)nfb / 4.0) + 1;
    G = G < 1 ? 1 : (G > kFbGridMax ? kFbGridMax : G);
    for (int d = 0; d < 3; d++) {
      const double e = rhi[d][0] - rlo[d][0];
      f->lo[d] = rlo[d][0];
      f->inv[d] = e > 0.0 ? (double)G / e : 0.0;
    }
    f->n = G;
    sG = G;
  }
  __syncthreads();
  const int G = sG, nc = G * G * G;
  const double l0 = f->lo[0], l1 = f->lo[1], l2 = f->lo[2];
  const double i0 = f->inv[0], i1 = f->inv[1], i2 = f->inv[2];
  for (int c = t; c < nc; c += nt) cur[c] = 0;
  __syncthreads();
  for (int j = t; j < nfb; j += nt) {
    double x[3];
    load_pt(qxyz, fb[j], x);
    const int c = fb_cell1(x[0], l0, i0, G) + G * (fb_cell1(x[1], l1, i1, G) + G * fb_cell1(x[2], l2, i2, G));
    atomicAdd(&cur[c], 1);
  }
  __threadfence_block();
  __syncthreads();
  if (t == 0) { // exclusive scan (at most kFbCells entries, once per call with fallbacks)
    int acc = 0;
    for (int c = 0; c < nc; c++) {
      const int v = cur[c];
      cells[c] = acc;
      cur[c] = acc;
      acc += v;
    }
    cells[nc] = acc;
  }
  __threadfence_block();
  __syncthreads();
  for (int j = t; j < nfb; j += nt) {
    double x[3];
    load_pt(qxyz, fb[j], x);
    const int c = fb_cell1(x[0], l0, i0, G) + G * (fb_cell1(x[1], l1, i1, G) + G * fb_cell1(x[2], l2, i2, G));
    items[atomicAdd(&cur[c], 1)] = j;
  }
}

// The query grid of a completed fallback list (cls 0: volume, 1: surface), one
// block, launched after the kernel that completes the list (r06: before, the
// last block of that kernel built it after a per-block ticket on one counter
// — k_bdy's 4096 tickets alone serialised ~47 us of atomics at the end of
// the surface branch, profiles/r06j); returns at once for an empty list
__global__ __launch_bounds__(kBlock) void k_fb_grid(const double *qxyz, const int *fb, DevStats *st, int cls,
                                                   FbGridBufs gb) {
  FbState *f = &st->fb[cls];
  const int nfb = f->nfb;
  if (nfb > 0) fb_grid_build(qxyz, fb, nfb, f, gb.cells, gb.cur, gb.items);
}

// the queries of the cells an element's (inflated) box covers: visit(j) for
// each list position j (the accept test itself); nothing when the box misses
// the grid's box
template <class F>
__device__ __forceinline__ void fb_grid_visit(const FbState *f, const int *cells, const int *items, const Box &b,
                                              F &&visit) {
  const int G = f->n;
  int a[3], e[3];
  for (int d = 0; d < 3; d++) {
    const double lo = f->lo[d], inv = f->inv[d];
    const double hi = inv > 0.0 ? lo + (double)G / inv : lo;
    if (b.hi[d] < lo || b.lo[d] > hi) return; // (NaN boxes: degenerate elements have infinite ones)
    a[d] = fb_cell1(b.lo[d], lo, inv, G);
    e[d] = fb_cell1(b.hi[d], lo, inv, G);
  }
  for (int z = a[2]; z <= e[2]; z++)
    for (int y = a[1]; y <= e[1]; y++)
      for (int x = a[0]; x <= e[0]; x++) {
        const int c = x + G * (y + G * z);
        for (int q = cells[c]; q < cells[c + 1]; q++) visit(items[q]);
      }
}

// ---------------------------------------------------------------- the two classes
//
// FbElem<NV>: one element of a class (NV = 4: a tetra against the volume
// queries, class 0; NV = 3: a tria against the surface queries, class 1) and
// everything the two kernels need to know about the class.  Constants: the
// hit codes, and the grid of both kernels, min(max_grid, max(min_grid, n /
// per_block)) & ~7 blocks for n elements (fixed by the background: the counts
// are on the device; a small group's empty launches cost their dispatch, r04l,
// cfg2: ~4 us each at 1024 blocks; trias are ~1-2 % of the tetra).
template <int NV>
struct FbElem;

// is element k in use?
template <int NV>
__device__ __forceinline__ bool fb_used(const Bg &bg, int k) {
  if constexpr (NV == 4) return tetv_row(bg, k).x > 0;
  else return bg.triv[3 * (size_t)(k - 1)] > 0;
}

// the vertices of element k (in use) to v and their coordinates, vertex by
// vertex, to dst[3 * NV]
template <int NV>
__device__ __forceinline__ void fb_load_pts(const Bg &bg, int k, int *v, double *dst) {
  if constexpr (NV == 4) {
    const int4 tv = tetv_row(bg, k);
    v[0] = tv.x, v[1] = tv.y, v[2] = tv.z, v[3] = tv.w;
  } else {
    const int *tv = bg.triv + 3 * (size_t)(k - 1);
    v[0] = tv[0], v[1] = tv[1], v[2] = tv[2];
  }
#pragma unroll
  for (int i = 0; i < NV; i++) load_pt(bg.xyz, v[i], dst + 3 * i);
}

template <>
struct FbElem<4> {
  static constexpr int cls = 0, max_grid = 1024, min_grid = 64, per_block = 16384;
  static constexpr int hit_accept = PMMG_HIT_VOL_EXHAUST, hit_closest = PMMG_HIT_VOL_CLOSEST;
  static constexpr int hit_stale = hit_closest; // (the volume has no second code)
  static __host__ __device__ __forceinline__ int count(const Bg &bg) { return bg.ne; }
  int v[4];
  double p[4][3];
  __device__ __forceinline__ void load(const Bg &bg, int k) { fb_load_pts<4>(bg, k, v, &p[0][0]); }
  __device__ __forceinline__ Box box(const Bg &) const {
    const double vol = orvol4(p[0], p[1], p[2], p[3]);
    return elem_box<4>(p, 0.0, !(fabs(vol) > 0.0) || !isfinite(vol));
  }
  // locate_pmmg.c:743-762
  __device__ __forceinline__ bool accepts(const Bg &, const double *x) const {
    double b[4];
    tet_bary(x, p[0], p[1], p[2], p[3], b);
    return min4(b) > -kEps;
  }
  __device__ __forceinline__ void accepted(const Bg &, const Slots &S, int ip, const double *x) const {
    double phi[4];
    tet_bary(x, p[0], p[1], p[2], p[3], phi);
    for (int s = 0; s < S.n; s++) interp_dyn<4>(S.s[s], ip, v, phi);
  }
  // the closest tetra's nearest vertex (PMMG_barycoord3d_getClosest)
  __device__ __forceinline__ int closest(const Bg &, const Slots &S, int ip, const double *x) const {
    double phi[4];
    closest_vertex<4>(x, p, phi);
    for (int s = 0; s < S.n; s++) interp_dyn<4>(S.s[s], ip, v, phi);
    return hit_closest;
  }
  static __device__ __forceinline__ double key(const double *x, const double (*q)[3]) {
    double b[4];
    const double vol = tet_bary(x, q[0], q[1], q[2], q[3], b);
    return fabs(min4(b)) * vol;
  }
};

template <>
struct FbElem<3> {
  static constexpr int cls = 1, max_grid = 256, min_grid = 32, per_block = 4096;
  static constexpr int hit_accept = PMMG_HIT_BDY_EXHAUST, hit_closest = PMMG_HIT_BDY_CLOSEST;
  static constexpr int hit_stale = PMMG_HIT_BDY_STALE;
  static __host__ __device__ __forceinline__ int count(const Bg &bg) { return bg.nt; }
  TriGeom t;
  __device__ __forceinline__ void load(const Bg &bg, int k) { tri_load(bg, k, t); }
  __device__ __forceinline__ Box box(const Bg &bg) const {
    return elem_box<3>(t.p, bg.hausd, !(t.q > 0.0) || !isfinite(t.q));
  }
  // locate_pmmg.c:483-503, with the vertices and area (pv, q) and the unit normal n; the coordinates in b
  static __device__ __forceinline__ bool test(const Bg &bg, const double *x, const double (*pv)[3], double q,
                                              const double *n, double *b) {
    const double dist = tri_bary(x, pv, q, n, b);
    const double bmin = fmin(b[0], fmin(b[1], b[2]));
    return bmin > -kEps && !(fabs(dist) > bg.hausd);
  }
  __device__ __forceinline__ bool accepts(const Bg &bg, const double *x) const {
    double b[3];
    return test(bg, x, t.p, t.q, t.n, b);
  }
  __device__ __forceinline__ void accepted(const Bg &, const Slots &S, int ip, const double *x) const {
    double phi[3];
    tri_bary(x, t.p, t.q, t.n, phi);
    interp_bdy(S, ip, t.v, phi, -1, -1);
  }
  // the reference's stale re-evaluation (locate_pmmg.c:505-509: vertices and
  // area of the last tria scanned, nt, with the closest tria's normal), else
  // the closest tria's nearest vertex
  __device__ __forceinline__ int closest(const Bg &bg, const Slots &S, int ip, const double *x) const {
    TriGeom ts;
    tri_load(bg, bg.nt, ts);
    double phi[3];
    int hit = hit_stale;
    if (!test(bg, x, ts.p, ts.q, t.n, phi)) {
      hit = hit_closest;
      closest_vertex<3>(x, t.p, phi);
    }
    interp_bdy(S, ip, t.v, phi, -1, -1);
    return hit;
  }
  // distance from x to the tria's centroid, in the arithmetic of the closest
  // tria search (locate_pmmg.c:400-416): x - sum_v p_v / 3, component by component
  static __device__ __forceinline__ double key(const double *x, const double (*q)[3]) {
    double d[3] = {x[0], x[1], x[2]};
    for (int v = 0; v < 3; v++)
      for (int c = 0; c < 3; c++) d[c] -= q[v][c] / 3.0;
    double nrm = 0;
    for (int c = 0; c < 3; c++) nrm += d[c] * d[c];
    return sqrt(nrm);
  }
};

// blocks of a class's two kernels on a background of n elements
template <int NV>
static inline int fb_blocks(long long n) {
  using E = FbElem<NV>;
  const long long b = n / E::per_block;
  return (int)(b < E::min_grid ? E::min_grid : b > E::max_grid ? E::max_grid : b) & ~7;
}

// one range's closest element of one query (closest scans with several ranges)
struct FbPart {
  double key;
  int idx;
  int pad;
};
// FbPart entries of a class (see ClosestSplit)
template <int NV>
constexpr size_t kFbPartCap = (size_t)kBlock * FbElem<NV>::max_grid;

// a finishing last block's hit counters (cnt[0]: code h0, cnt[1]: code h1), flushed once
__device__ __forceinline__ void count_hits_flush(unsigned *cnt, DevStats *st, int h0, int h1) {
  __syncthreads();
  if (threadIdx.x == 0) {
    if (cnt[0]) atomicAdd(&stat_part(st)->cnt[h0], (unsigned long long)cnt[0]);
    if (cnt[1]) atomicAdd(&stat_part(st)->cnt[h1], (unsigned long long)cnt[1]);
  }
}

// ---------------------------------------------------------------- accept scan

// The lowest-index element accepting each fallback query of the class, each
// element tested against the queries of the grid cells its inflated box
// covers; the last block interpolates the accepted ones and lists the others
// (nac)
template <int NV>
__global__ __launch_bounds__(kBlock) void k_exhaust_accept(Bg bg, const double *qxyz, const int *fb, DevStats *st,
                                                           int *best, int *nac, const int *gcells, const int *gitems,
                                                           Slots S, int *elem_out, int8_t *hit_out) {
  using E = FbElem<NV>;
  FbState *f = &st->fb[E::cls];
  const int nfb = f->nfb;
  if (nfb == 0) return;
  // each XCD a contiguous eighth of the elements (shared vertex rows in its L2)
  const XcdChunk ch = xcd_chunk(E::count(bg));
  for (int it = 0; it < ch.iters; it++) {
    const long long j0 = ch.start + it * ch.stride;
    if (j0 >= ch.hi) break;
    const int k = (int)(j0 + 1);
    if (!fb_used<NV>(bg, k)) continue;
    E e;
    e.load(bg, k);
    const Box box = e.box(bg);
    fb_grid_visit(f, gcells, gitems, box, [&](int j) {
      double x[3];
      load_pt(qxyz, fb[j], x);
      if (!in_box(box, x) || best[j] <= k) return; // (a stale read only costs a test)
      if (e.accepts(bg, x)) atomicMin(&best[j], k);
    });
  }
  if (!last_block(&f->done[0], true)) return; // (only when there are fallbacks)
  __shared__ int s_nac;
  __shared__ unsigned s_cnt[2];
  if (threadIdx.x == 0) {
    s_nac = 0;
    s_cnt[0] = s_cnt[1] = 0u;
  }
  __syncthreads();
  for (int j = threadIdx.x; j < nfb; j += blockDim.x) {
    const int k = load_agent(&best[j]);
    if (k == INT_MAX) {
      nac[atomicAdd(&s_nac, 1)] = j;
      continue;
    }
    const int ip = fb[j];
    double x[3];
    load_pt(qxyz, ip, x);
    E e;
    e.load(bg, k);
    e.accepted(bg, S, ip, x);
    if (elem_out) elem_out[ip - 1] = k;
    if (hit_out) hit_out[ip - 1] = (int8_t)E::hit_accept;
    atomicAdd(&s_cnt[0], 1u);
  }
  __syncthreads();
  if (threadIdx.x == 0) f->nac = s_nac;
  count_hits_flush(s_cnt, st, E::hit_accept, E::hit_accept);
}

// ---------------------------------------------------------------- closest scan

// How a closest scan deals n queries to a grid of G blocks of 256 lanes:
// groups of Qp queries (Qp = 256, or the next power of two >= n for a short
// list, whose queries then get lpq = 256 / Qp lanes each, every lane taking
// every lpq-th element of a tile), and per group nr ranges of consecutive
// elements (one block each).  n * nr <= G * 256 (<= kFbPartCap of the
// class), the partial minima's buffer.
struct ClosestSplit {
  int Qp, lpq, nqg, nr;
};
__device__ __forceinline__ ClosestSplit closest_split(int n, int G) {
  ClosestSplit s;
  if (n >= kBlock) {
    s.Qp = kBlock;
    s.lpq = 1;
    s.nqg = (n + kBlock - 1) / kBlock;
  } else {
    s.Qp = 1;
    while (s.Qp < n) s.Qp <<= 1;
    s.lpq = kBlock / s.Qp;
    s.nqg = 1;
  }
  s.nr = s.nqg >= G ? 1 : G / s.nqg;
  return s;
}

// (key, index) order of the closest searches: the lowest index at the minimum
// key, starting from (1e10, index 0); a NaN key never wins.  This is the
// reference's exhaustive scan on its own (it keeps the first element strictly
// closer while scanning in index order, src/locate_pmmg.c:753-765) but not its
// whole rule: the reference seeds closestDist / closestTet with what its walk
// met (:800-815, :864) and skips the walk's visited tetra (:753), so on an
// exact key tie between a walked element and a lower-index one it returns the
// walked one.  Listed as a known divergence (ties of the closest
// metric are broken by lowest index); only exact ties of |min bary| * vol
// for points outside every element can differ.
__device__ __forceinline__ bool key_before(double ka, int ia, double kb, int ib) {
  return ka < kb || (ka == kb && ia < ib);
}

// The closest element (FbElem<NV>::key: tetra |bary_min| * vol, tria centroid
// distance) of each query of the list nac[0, n), by ranges.  Returns (in the
// block's lanes with sub == 0) the range's minimum of query qi; the caller
// stores it.
template <int NV>
__device__ __forceinline__ void closest_range(const Bg &bg, const double *x, bool active, int lpq, int sub, int k0,
                                              int k1, double &bkey, int &bidx, double (*tp)[3 * NV], int *tk) {
  constexpr int kTile = kBlock;
  for (int t0 = k0; t0 < k1; t0 += kTile) {
    __syncthreads();
    {
      const int k = t0 + (int)threadIdx.x;
      const bool used = k < k1 && fb_used<NV>(bg, k);
      int v[NV];
      if (used) fb_load_pts<NV>(bg, k, v, tp[threadIdx.x]);
      tk[threadIdx.x] = used ? k : 0;
    }
    __syncthreads();
    if (!active) continue;
    const int nt = min(kTile, k1 - t0);
    for (int t = sub; t < nt; t += lpq) {
      const int k = tk[t];
      if (k == 0) continue;
      double p[NV][3];
#pragma unroll
      for (int v = 0; v < NV; v++)
#pragma unroll
        for (int c = 0; c < 3; c++) p[v][c] = tp[t][3 * v + c];
      const double key = FbElem<NV>::key(x, p);
      if (key < bkey) { // index order within a lane: strict, as the reference
        bkey = key;
        bidx = k;
      }
    }
  }
}

// the closest scan's body: every block's groups and ranges, the lanes of a
// query merged in LDS, the range minima stored (part) or, with one range,
// the result itself (res)
template <int NV>
__device__ __forceinline__ void closest_scan(const Bg &bg, const double *qxyz, const int *fb, const int *nac, int n,
                                             int nelem, FbPart *part, int *res) {
  __shared__ double tp[kBlock][3 * NV];
  __shared__ int tk[kBlock];
  __shared__ double mk[kBlock];
  __shared__ int mi[kBlock];
  const ClosestSplit sp = closest_split(n, (int)gridDim.x);
  const int qsub = (int)threadIdx.x % sp.Qp, sub = (int)threadIdx.x / sp.Qp;
  const int nwork = sp.nqg * sp.nr;
  for (int w = blockIdx.x; w < nwork; w += gridDim.x) {
    const int g = w % sp.nqg, r = w / sp.nqg;
    const int qi = g * sp.Qp + qsub;
    const bool active = qi < n;
    double x[3] = {0.0, 0.0, 0.0};
    if (active) load_pt(qxyz, fb[nac[qi]], x);
    const int k0 = 1 + (int)((long long)nelem * r / sp.nr), k1 = 1 + (int)((long long)nelem * (r + 1) / sp.nr);
    double bkey = 1.0e10;
    int bidx = 0;
    closest_range<NV>(bg, x, active, sp.lpq, sub, k0, k1, bkey, bidx, tp, tk);
    if (sp.lpq > 1) {
      __syncthreads();
      mk[threadIdx.x] = bkey;
      mi[threadIdx.x] = bidx;
      __syncthreads();
      if (sub == 0)
        for (int s = 1; s < sp.lpq; s++) {
          const int o = qsub + s * sp.Qp;
          if (key_before(mk[o], mi[o], bkey, bidx)) {
            bkey = mk[o];
            bidx = mi[o];
          }
        }
    }
    if (active && sub == 0) {
      if (sp.nr == 1) res[qi] = bidx;
      else part[(long long)r * (sp.nqg * sp.Qp) + qi] = FbPart{bkey, bidx, 0};
    }
  }
}

// the last block: query qi's closest element over the ranges
__device__ __forceinline__ int closest_result(int qi, int n, const FbPart *part, const int *res) {
  const ClosestSplit sp = closest_split(n, (int)gridDim.x);
  if (sp.nr == 1) return load_agent(&res[qi]);
  double bkey = 1.0e10;
  int bidx = 0;
  for (int r = 0; r < sp.nr; r++) { // ranges in index order
    const FbPart e = part[(long long)r * (sp.nqg * sp.Qp) + qi];
    if (key_before(e.key, e.idx, bkey, bidx)) {
      bkey = e.key;
      bidx = e.idx;
    }
  }
  return bidx;
}

// The closest element of the class's queries nothing accepted, then (last
// block) what the reference makes of it (FbElem<NV>::closest) and the
// interpolation
template <int NV>
__global__ __launch_bounds__(kBlock) void k_exhaust_closest(Bg bg, const double *qxyz, const int *fb, DevStats *st,
                                                            const int *nac, FbPart *part, int *res, Slots S,
                                                            int *elem_out, int8_t *hit_out) {
  using E = FbElem<NV>;
  FbState *f = &st->fb[E::cls];
  const int n = f->nac;
  if (n == 0) return;
  closest_scan<NV>(bg, qxyz, fb, nac, n, E::count(bg), part, res);
  if (!last_block(&f->done[1], true)) return; // (only when there are fallbacks)
  __shared__ unsigned s_cnt[2];
  if (threadIdx.x == 0) s_cnt[0] = s_cnt[1] = 0u;
  __syncthreads();
  for (int qi = threadIdx.x; qi < n; qi += blockDim.x) {
    const int k = closest_result(qi, n, part, res);
    if (k <= 0) continue; // no element closer than the reference's 1e10 start
    const int ip = fb[nac[qi]];
    double x[3];
    load_pt(qxyz, ip, x);
    E e;
    e.load(bg, k);
    const int hit = e.closest(bg, S, ip, x);
    if (elem_out) elem_out[ip - 1] = k;
    if (hit_out) hit_out[ip - 1] = (int8_t)hit;
    atomicAdd(&s_cnt[hit == E::hit_closest ? 0 : 1], 1u);
  }
  count_hits_flush(s_cnt, st, E::hit_closest, E::hit_stale);
}

} // namespace pmmg
