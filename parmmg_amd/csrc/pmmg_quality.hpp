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
// host's).  Shared by the metis weights (pmmg_quality.hip) and the edge-length
// report (pmmg_meshstats.hip): both must be built with -ffp-contract=off.
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
