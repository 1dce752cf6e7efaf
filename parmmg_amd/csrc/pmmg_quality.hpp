// pmmg_quality.hpp — internal interface of pmmg_quality.hip (tetra quality in
// the interpolated metric); the C-ABI wrapper lives in pmmg_hip.hip.
#pragma once
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

// qual[ne] and the minimum over used tetra (bit pattern of a non-negative
// double, all ones when no tetra is used) in *h_minbits; device pointers
// except h_minbits (pinned or pageable host).  Synchronous.  Returns 1/0.
int pmmg_qual_tetra(hipStream_t s, int np, const double *xyz, int ne, const int *tetv, int met_size,
                    const double *met, double *qual, unsigned long long *d_minbits, unsigned long long *h_minbits);

// PMMG_computeWgt_mesh / PMMG_computeWgt on device arrays (tetv, ftag 16-byte /
// 8-byte aligned); synchronous; 1/0
int pmmg_wgt_mesh(hipStream_t s, const double *xyz, int ne, const int *tetv, const int *xt, const uint16_t *ftag,
                  int met_size, const double *met, int tag, double *qual);
int pmmg_wgt_faces(hipStream_t s, const double *xyz, const int *tetv, int nface, const int *face, int met_size,
                   const double *met, double *wgt);

// MMG5_lenedgCoor_iso / MMG5_lenedgCoor_ani of Mmg @889d408, restated (aniso
// ridge-point storage not modelled), in the operation order of
// oracle/pmmg_oracle.c; log1p is the device library's (within an ulp of the
// host's).  Shared by the metis weights (pmmg_quality.hip, pmmg_graph.hip) and the
// edge-length report (pmmg_meshstats.hip): all must be built with -ffp-contract=off.
constexpr double kMmgEps = 1.0e-06; // MMG5_EPS

__device__ __forceinline__ double lenedg_iso(const double *ca, const double *cb, double h1, double h2) {
  double l = (cb[0] - ca[0]) * (cb[0] - ca[0]) + (cb[1] - ca[1]) * (cb[1] - ca[1]) + (cb[2] - ca[2]) * (cb[2] - ca[2]);
  l = sqrt(l);
  const double r = h2 / h1 - 1.0;
  return (fabs(r) < kMmgEps) ? (l / h1) : (l / (h2 - h1) * log1p(r));
}

__device__ __forceinline__ double lenedg_ani(const double *ca, const double *cb, const double *sa, const double *sb) {
  const double ux = cb[0] - ca[0], uy = cb[1] - ca[1], uz = cb[2] - ca[2];
  double dd1 = sa[0] * ux * ux + sa[3] * uy * uy + sa[5] * uz * uz + 2.0 * (sa[1] * ux * uy + sa[2] * ux * uz + sa[4] * uy * uz);
  if (dd1 <= 0.0) dd1 = 0.0;
  double dd2 = sb[0] * ux * ux + sb[3] * uy * uy + sb[5] * uz * uz + 2.0 * (sb[1] * ux * uy + sb[2] * ux * uz + sb[4] * uy * uz);
  if (dd2 <= 0.0) dd2 = 0.0;
  if (fabs(dd1 - dd2) < 0.05) return sqrt(0.5 * (dd1 + dd2));
  return (sqrt(dd1) + sqrt(dd2) + 4.0 * sqrt(0.5 * (dd1 + dd2))) / 6.0;
}

// PMMG_computeWgt (src/metis_pmmg.c:280-300) of face ifac of the tetra with vertices v (1-based), in the
// operation order of oracle/pmmg_oracle.c orc_face_wgt.  Shared by the interface weights (pmmg_quality.hip)
// and the METIS element graph (pmmg_graph.hip), which takes a tetra's six edge lengths once and sums each
// face's three terms in the kIarf order used here, so both give the same bits.
constexpr double kHugeWgt = 1000000.0; // PMMG_WGTVAL_HUGEINT
static constexpr int kIare[6][2] = {{0, 1}, {0, 2}, {0, 3}, {1, 2}, {1, 3}, {2, 3}}; // MMG5_iare
static constexpr int kIarf[4][3] = {{5, 4, 3}, {5, 1, 2}, {4, 2, 0}, {3, 0, 1}};     // MMG5_iarf

// one edge's term of the face sum
__device__ __forceinline__ double wgt_term(double len) { return len <= 1.0 ? len - 1.0 : 1.0 / len - 1.0; }

// the weight from the finished sum
__device__ __forceinline__ double wgt_of_res(double res) {
  const double w = 1.0 / exp(28.0 * res / 3.0);
  return w < kHugeWgt ? w : kHugeWgt;
}

__device__ inline double face_wgt(const double *xyz, const int *v, int ifac, int met_size, const double *met) {
  if (met_size != 1 && met_size != 6) return kHugeWgt;
  double res = 0.0;
  for (int i = 0; i < 3; i++) {
    const int ia = kIarf[ifac][i];
    const int ip1 = v[kIare[ia][0]], ip2 = v[kIare[ia][1]];
    const double *ca = xyz + 3 * (size_t)(ip1 - 1), *cb = xyz + 3 * (size_t)(ip2 - 1);
    const double len = met_size == 1 ? lenedg_iso(ca, cb, met[ip1 - 1], met[ip2 - 1])
                                     : lenedg_ani(ca, cb, met + 6 * (size_t)(ip1 - 1), met + 6 * (size_t)(ip2 - 1));
    res += wgt_term(len);
  }
  return wgt_of_res(res);
}
