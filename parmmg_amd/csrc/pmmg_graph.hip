// pmmg_graph.hip — the METIS element graph of a group and its metric
// weights, on the device.
//
// PMMG_graph_meshElts2metis (reference src/metis_pmmg.c:746-823, called from
// PMMG_part_meshElts2metis :1293 by the group split and the distribution)
// turns the tetra adjacency into the CSR dual graph METIS partitions: xadj,
// adjncy = the neighbours of every tetra in (tetra, face) order and, during
// the iterations, adjwgt = max((int)PMMG_computeWgt(face), 1).  The adapted
// mesh and its interpolated metric are in HBM after a transfer, so the graph
// is built where they are.
//
// Two passes, one lane per tetra, block b = tetra 256 b ... 256 b + 255:
//   count  the links of a row are range-checked and counted, each block
//          leaves one partial; an exclusive scan over the partials (hipcub)
//          gives every block its base offset and the total;
//   fill   a tetra's six edge lengths are taken once and each linked face
//          sums its three terms in MMG5_iarf order (face_wgt's order: the
//          same bits, pmmg_quality.hpp); the block's entries are compacted
//          in LDS at the position the global array gives them modulo 4 words
//          and leave as one contiguous run per array, 16 bytes per lane
//          between an unaligned head and tail of at most 3 words.
// Rows have 0 to 4 entries, so a lane's own offset is data dependent: stored
// from the lanes directly the entries would leave as scattered 4-byte words.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>
#include <stdio.h>

#include "pmmg_graph.hpp"
#include "pmmg_devutil.hpp"
#include "pmmg_quality.hpp"

namespace {

constexpr int kGBlock = 256;
constexpr int kGWaves = kGBlock / 64;
constexpr int kGEntries = 4 * kGBlock; // graph entries of a block at most

// the call's own flag bit, beside the MESH_ bits of pmmg_devutil.hpp
enum { G_BADID = 2 };

// Count pass.  btot[b]: graph entries of block b.  A used row (tetv NULL: every row) counts its non-zero
// links; an unused one (v[0] <= 0) is an empty row whatever its links hold.  flags: a link out of range,
// a vertex id of a used tetra outside [1, np_check] (np_check 0: not looked at), an unused row seen.
__global__ __launch_bounds__(kGBlock) void k_graph_count(int ne, const int4 *tetv, int tstride, const int4 *adja,
                                                         int astride, int np_check, int *btot, int *flags) {
  __shared__ int wt[kGWaves];
  __shared__ int sflag;
  if (threadIdx.x == 0) sflag = 0;
  __syncthreads();
  const long long k = (long long)blockIdx.x * kGBlock + threadIdx.x;
  int c = 0, bad = 0;
  if (k < ne) {
    bool used = true;
    if (tetv) {
      const int4 v = tetv[(size_t)k * tstride];
      used = v.x > 0;
      if (!used)
        bad |= MESH_UNUSED;
      else if (np_check && (v.x > np_check || v.y < 1 || v.y > np_check || v.z < 1 || v.z > np_check || v.w < 1 ||
                            v.w > np_check))
        bad |= G_BADID;
    }
    if (used) {
      const int4 a = adja[(size_t)k * astride];
      const int lk[4] = {a.x, a.y, a.z, a.w};
#pragma unroll
      for (int f = 0; f < 4; f++)
        if (lk[f]) {
          if (link_ok(lk[f], ne))
            c++;
          else
            bad |= MESH_BADLINK;
        }
    }
  }
  if (bad) atomicOr(&sflag, bad);
  const int n = block_reduce<kGWaves>(c, wt, IntSum());
  if (threadIdx.x == 0) {
    btot[blockIdx.x] = n;
    if (sflag) atomicOr(flags, sflag);
  }
}

// words [lo, hi) of the block's LDS array to g, word j to g[j]; g is 16-byte aligned, so the whole quads
// in the range go as 16-byte stores and at most 3 words before and after them as single ones
__device__ __forceinline__ void flush_run(const int *s, int *g, int lo, int hi) {
  const int q0 = (lo + 3) >> 2, q1 = hi >> 2; // whole quads [q0, q1)
  for (int q = q0 + (int)threadIdx.x; q < q1; q += kGBlock)
    reinterpret_cast<int4 *>(g)[q] = reinterpret_cast<const int4 *>(s)[q];
  const int head_end = 4 * q0 < hi ? 4 * q0 : hi;
  const int tail_lo = 4 * q1 > 4 * q0 ? 4 * q1 : 4 * q0;
  const int j = lo + (int)threadIdx.x;
  if (j < head_end) g[j] = s[j];
  const int t = tail_lo + (int)threadIdx.x;
  if (t < hi) g[t] = s[t];
}

enum { W_NONE = 0, W_ISO = 1, W_HUGE = 2, W_ANI = 6 };

// Fill pass.  boff[b]: entries before block b.  xadj[k + 1] = entries of rows 0 .. k (consecutive lanes,
// consecutive words).  adjncy NULL: xadj only (the caller's arrays are too small).  MODE W_NONE: no
// weights, neither xyz nor met is read, and tetv only when the count pass saw an unused row (else NULL).
template <int MODE>
__global__ __launch_bounds__(kGBlock) void k_graph_fill(const double *xyz, int ne, const int4 *tetv, int tstride,
                                                        const int4 *adja, int astride, const double *met,
                                                        const int *boff, int *xadj, int *adjncy, int *adjwgt) {
  __shared__ __attribute__((aligned(16))) int s_adj[kGEntries + 4];
  __shared__ __attribute__((aligned(16))) int s_wgt[MODE != W_NONE ? kGEntries + 4 : 4];
  __shared__ int wt[kGWaves];
  const long long k = (long long)blockIdx.x * kGBlock + threadIdx.x;
  bool used = k < ne;
  int4 v = make_int4(0, 0, 0, 0);
  if (used && tetv) {
    v = tetv[(size_t)k * tstride];
    used = v.x > 0;
  }
  int4 a = make_int4(0, 0, 0, 0);
  if (used) a = adja[(size_t)k * astride];
  const int lk[4] = {a.x, a.y, a.z, a.w};
  const int c = (a.x != 0) + (a.y != 0) + (a.z != 0) + (a.w != 0);
  int n;
  const int pos = block_prefix<kGWaves>(c, wt, &n);
  const int base = boff[blockIdx.x];
  if (k < ne) xadj[k + 1] = base + pos + c;
  if (k == 0) xadj[0] = 0;
  if (!adjncy) return;
  // the LDS arrays start at the 16-byte line of the block's first global word
  const int oa = (int)(((uintptr_t)(adjncy + base) >> 2) & 3);
  const int ow = MODE != W_NONE ? (int)(((uintptr_t)(adjwgt + base) >> 2) & 3) : 0;
  if (c) {
    int wi[4] = {1, 1, 1, 1};
    if (MODE == W_HUGE) {
#pragma unroll
      for (int f = 0; f < 4; f++) wi[f] = (int)kHugeWgt;
    }
    if (MODE == W_ISO || MODE == W_ANI) {
      const int id[4] = {v.x, v.y, v.z, v.w};
      double p[4][3];
#pragma unroll
      for (int i = 0; i < 4; i++)
#pragma unroll
        for (int j = 0; j < 3; j++) p[i][j] = xyz[3 * (size_t)(id[i] - 1) + j];
      double term[6]; // the six edges once, each with face_wgt's arguments for that edge
      if (MODE == W_ISO) {
        double h[4];
#pragma unroll
        for (int i = 0; i < 4; i++) h[i] = met[id[i] - 1];
#pragma unroll
        for (int ia = 0; ia < 6; ia++)
          term[ia] = wgt_term(lenedg_iso(p[kIare[ia][0]], p[kIare[ia][1]], h[kIare[ia][0]], h[kIare[ia][1]]));
      } else {
        double m[4][6];
#pragma unroll
        for (int i = 0; i < 4; i++)
#pragma unroll
          for (int j = 0; j < 6; j++) m[i][j] = met[6 * (size_t)(id[i] - 1) + j];
#pragma unroll
        for (int ia = 0; ia < 6; ia++)
          term[ia] = wgt_term(lenedg_ani(p[kIare[ia][0]], p[kIare[ia][1]], m[kIare[ia][0]], m[kIare[ia][1]]));
      }
#pragma unroll
      for (int f = 0; f < 4; f++) {
        if (!lk[f]) continue; // (a boundary face's weight is not finished)
        double res = 0.0;
#pragma unroll
        for (int i = 0; i < 3; i++) res += term[kIarf[f][i]];
        const double w = wgt_of_res(res);
        wi[f] = w >= 1.0 ? (int)w : 1; // max((int)w, 1); w <= PMMG_WGTVAL_HUGEINT; a NaN gives 1
      }
    }
    int j = pos;
#pragma unroll
    for (int f = 0; f < 4; f++)
      if (lk[f]) {
        s_adj[oa + j] = lk[f] / 4 - 1;
        if (MODE != W_NONE) s_wgt[ow + j] = wi[f];
        j++;
      }
  }
  __syncthreads();
  flush_run(s_adj, adjncy + base - oa, oa, oa + n);
  if (MODE != W_NONE) flush_run(s_wgt, adjwgt + base - ow, ow, ow + n);
}

} // namespace

int pmmg_graph_metis(hipStream_t s, int np, const double *xyz, TetView m, int want_wgt, int met_size,
                     const double *met, int cap, int64_t *nadjncy, int *xadj, int *adjncy, int *adjwgt,
                     GraphCache *cache, SnapCache *snap, char *msg, size_t msglen) {
  *nadjncy = 0;
  const int ne = m.ne;
  if (ne == 0) {
    DEVCK(hipMemsetAsync(xadj, 0, sizeof(int), s));
    DEVCK(hipStreamSynchronize(s));
    return 1;
  }
  // MMG3D_hashTetra's branch of src/metis_pmmg.c:756
  if (!m.adja && !built_adjacency(s, "metis_graph", np, &m, cache->adja, snap, msg, msglen)) return 0;
  const int tstride = m.tstride, astride = m.astride;
  const int4 *tv = reinterpret_cast<const int4 *>(m.tetv), *av = reinterpret_cast<const int4 *>(m.adja);
  const int nblk = (ne + kGBlock - 1) / kGBlock;
  const char *oom = "metis_graph: out of device memory (block counts)";
  int *flags = get<int>(cache->flags, 4);
  if (!flags) return refuse(msg, msglen, oom);
  if (!reserve(cache->rows, nblk, s, oom, msg, msglen)) return 0; // (ahead of the count kernel)
  int *btot = cache->rows.btot.as<int>(), *boff = cache->rows.boff.as<int>();
  DEVCK(hipMemsetAsync(flags, 0, 4 * sizeof(int), s));
  hipLaunchKernelGGL(k_graph_count, dim3(nblk), dim3(kGBlock), 0, s, ne, tv, tstride, av, astride, want_wgt ? np : 0,
                     btot, flags);
  DEVCK(hipGetLastError());
  int h_flags = 0, h_total = 0;
  DEVCK(hipMemcpyAsync(&h_flags, flags, sizeof(int), hipMemcpyDeviceToHost, s)); // (back with the total)
  if (!offsets(cache->rows, s, nblk, &h_total, msg, msglen)) return 0;
  if (h_flags & MESH_BADLINK) {
    snprintf(msg, msglen, "metis_graph: an adja entry lies outside [4, 4*%d+3] (nothing written to the lists)", ne);
    return 0;
  }
  if (h_flags & G_BADID) {
    snprintf(msg, msglen, "metis_graph: a used tetra has a vertex id outside [1, %d] (nothing written to the lists)",
             np);
    return 0;
  }
  const char *tail = ": the mesh must be packed (nothing written to the lists)";
  if (!check_links<kGBlock>(s, "metis_graph", tail, m, flags, &h_flags, msg, msglen)) return 0;
  *nadjncy = h_total;
  const bool lists = h_total <= cap;
  int *oa = lists ? adjncy : nullptr;
  const int mode = !want_wgt ? W_NONE : (met_size == 1 ? W_ISO : (met_size == 6 ? W_ANI : W_HUGE));
  // without weights the rows' vertices are read only where the count pass saw an unused row
  const int4 *tf = (mode != W_NONE || (h_flags & MESH_UNUSED)) ? tv : nullptr;
#define FILL(M)                                                                                              \
  hipLaunchKernelGGL(k_graph_fill<M>, dim3(nblk), dim3(kGBlock), 0, s, xyz, ne, tf, tstride, av, astride, met, boff, \
                     xadj, oa, adjwgt)
  switch (mode) {
    case W_NONE: FILL(W_NONE); break;
    case W_ISO: FILL(W_ISO); break;
    case W_ANI: FILL(W_ANI); break;
    default: FILL(W_HUGE); break;
  }
#undef FILL
  DEVCK(hipGetLastError());
  DEVCK(hipStreamSynchronize(s));
  if (!lists) {
    snprintf(msg, msglen, "metis_graph: %d graph entries exceed cap = %d (nothing written to the lists)", h_total, cap);
    return 0;
  }
  return 1;
}
