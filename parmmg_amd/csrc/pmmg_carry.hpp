// pmmg_carry.hpp — the carry-over of a host-mode call's new points and
// written rows into the next background (included by pmmg_hip.hip only; the
// entry points pmmg_hip_keep / pmmg_hip_carry_over are there).
#pragma once

#include "pmmg_xfer.hpp"

// ---------------------------------------------------------------- carry-over
//
// ParMmg's next iteration takes the adapted group as its old group
// (src/libparmmg1.c:653 -> PMMG_update_oldGrps, src/grpsplit_pmmg.c:1224-1248):
// its vertices are the new points the transfer step just located and its
// solutions the rows the step just wrote, both still in HBM after a
// host-mode call.  pmmg_hip_keep keeps them (the staging buffers are swapped
// into a slot, no copy); pmmg_hip_carry_over arms the next host-mode
// set_background / set_solutions to take from the slot every row it holds —
// vertex i + 1 of the new background is kept point src[i] — and to upload only
// the rest: vertices not in the slot (src[i] == 0, e.g. moved in by load
// balancing) and rows the step did not write (skipped points, whose values
// the caller copies on the host, and MMG5_invmat failures), found on the
// device by the output sentinel.

// (extern "C": the two kernels keep the unmangled names they had among the entry points)
// to[i] = from[src[i] - 1] (row doubles; src NULL: the identity, to NULL: no
// copy); need[i] = 1 where the row must come from the host: src[i] == 0, or
// (check) the kept row is the unwritten sentinel
extern "C" __global__ void k_carry_gather(const double *from, int row, const int *src, long long np, double *to,
                                          uint8_t *need, int check) {
  for (long long i = blockIdx.x * (long long)blockDim.x + threadIdx.x; i < np; i += (long long)gridDim.x * blockDim.x) {
    const long long s = src ? (long long)src[i] : i + 1;
    bool miss = s <= 0;
    if (!miss) {
      const double *f = from + (size_t)row * (size_t)(s - 1);
      miss = check && (unsigned long long)__double_as_longlong(f[0]) == kSentinel;
      if (!miss && to)
        for (int j = 0; j < row; j++) to[(size_t)row * (size_t)i + j] = f[j];
    }
    if (miss && need) need[i] = 1;
  }
}

// to[ids[k] - 1] = rows[k] (row doubles), k < *n
extern "C" __global__ void k_scatter_rows(const double *rows, const int *ids, const int *n, int row, double *to) {
  for (long long k = blockIdx.x * (long long)blockDim.x + threadIdx.x; k < *n; k += (long long)gridDim.x * blockDim.x)
    for (int j = 0; j < row; j++) to[(size_t)row * (size_t)(ids[k] - 1) + j] = rows[(size_t)row * (size_t)k + j];
}

// host rows ids (1-based) of `host` uploaded and scattered into dst
static int carry_host_rows(pmmg_hip_ctx *c, const std::vector<int> &ids, const double *host, int row, double *dst) {
  if (ids.empty()) return 1;
  std::vector<double> rows((size_t)row * ids.size());
  for (size_t k = 0; k < ids.size(); k++)
    memcpy(&rows[(size_t)row * k], host + (size_t)row * (size_t)(ids[k] - 1), sizeof(double) * row);
  const int n = (int)ids.size();
  if (!upload(c, c->carry_rows, rows.data(), sizeof(double) * rows.size()) ||
      !upload(c, c->carry_ids, ids.data(), sizeof(int) * ids.size()) || !upload(c, c->carry_cnt, &n, sizeof(int)))
    return 0;
  hipLaunchKernelGGL(k_scatter_rows, dim3(blocks_for(n, 4096)), dim3(kBlock), 0, c->stream,
                     c->carry_rows.as<const double>(), c->carry_ids.as<const int>(), c->carry_cnt.as<const int>(), row,
                     dst);
  HIPCK(c, hipGetLastError());
  return 1;
}

static void carry_disarm(pmmg_hip_ctx *c) {
  c->carry_slot = -1;
  c->carry_bg = false;
  c->carry_src.clear();
}

// set_background, host mode, carry armed: the vertices from the slot
static int carry_vertices(pmmg_hip_ctx *c, int np, const double *xyz) {
  pmmg_hip_ctx::Kept &k = c->kept[c->carry_slot];
  if (np != c->carry_np || c->carry_bg) {
    set_err(c, "set_background: the armed carry-over is for %d vertices (got %d)%s", c->carry_np, np,
            c->carry_bg ? " and was taken already" : "");
    carry_disarm(c);
    return 0;
  }
  k.valid = false; // the slot is consumed by this carry, whatever happens next (a swapped-out
                   // buffer must never feed a later carry of the same slot)
  if (c->carry_src.empty()) {
    std::swap(c->o_xyz, k.xyz); // every row is a kept point, in order
  } else {
    if (!ensure(c, c->o_xyz, sizeof(double) * 3 * (size_t)np) ||
        !upload(c, c->carry_dsrc, c->carry_src.data(), sizeof(int) * (size_t)np)) {
      carry_disarm(c);
      return 0;
    }
    hipLaunchKernelGGL(k_carry_gather, dim3(blocks_for(np, 4096)), dim3(kBlock), 0, c->stream,
                       k.xyz.as<const double>(), 3, c->carry_dsrc.as<const int>(), (long long)np, c->o_xyz.as<double>(),
                       (uint8_t *)nullptr, 0);
    std::vector<int> ids;
    for (int i = 0; i < np; i++)
      if (c->carry_src[i] == 0) ids.push_back(i + 1);
    if (!carry_host_rows(c, ids, xyz, 3, c->o_xyz.as<double>())) {
      carry_disarm(c);
      return 0;
    }
  }
  c->carry_bg = true;
  return 1;
}

// set_solutions, host mode, carry armed: the metric and the fields whose
// sizes match the kept ones from the slot, their missing rows from the host
static int carry_solutions_body(pmmg_hip_ctx *c, int met_size, const double *met, int nfield, const int *field_size,
                                const double *const *fields) {
  pmmg_hip_ctx::Kept &k = c->kept[c->carry_slot];
  const int np = c->carry_np;
  const bool ident = c->carry_src.empty();
  hipStream_t s = c->stream;
  if (!c->carry_bg || np != c->bg.np) {
    set_err(c, "set_solutions: the armed carry-over needs set_background with its %d vertices first", np);
    carry_disarm(c);
    return 0;
  }
  const long long ncls = np / kScanChunk + 1;
  if (!ensure(c, c->carry_need, (size_t)np) || !ensure(c, c->carry_ids, sizeof(int) * (size_t)np) ||
      !ensure(c, c->carry_cnt, sizeof(int)) || !ensure(c, c->carry_bc, sizeof(int) * (size_t)ncls))
    return 0;
  HIPCK(c, hipMemsetAsync(c->carry_need.p, 0, (size_t)np, s));
  struct Arr { DevBuf *dst; const double *host; int row; };
  std::vector<Arr> carried;
  uint8_t *const need = c->carry_need.as<uint8_t>();
  // one solution array into dst and its address into *dev: from the slot's `from` when it is kept there with the
  // same row size (its missing rows are fetched below), else up whole from the host through the copy stream
  auto take = [&](DevBuf &dst, DevBuf *from, const double *host, int row, const double **dev) -> int {
    if (!from || !from->p)
      return copy_stream(c) &&
             take_input(c, PMMG_HIP_HOST, host, sizeof(double) * row * (size_t)np, dst, dev, c->cstream);
    if (ident) {
      std::swap(dst, *from);
      hipLaunchKernelGGL(k_carry_gather, dim3(blocks_for(np, 4096)), dim3(kBlock), 0, s, dst.as<const double>(), row,
                         (const int *)nullptr, (long long)np, (double *)nullptr, need, 1);
    } else {
      if (!ensure(c, dst, sizeof(double) * row * (size_t)np)) return 0;
      hipLaunchKernelGGL(k_carry_gather, dim3(blocks_for(np, 4096)), dim3(kBlock), 0, s, from->as<const double>(), row,
                         c->carry_dsrc.as<const int>(), (long long)np, dst.as<double>(), need, 1);
    }
    HIPCK(c, hipGetLastError());
    carried.push_back(Arr{&dst, host, row});
    *dev = dst.as<const double>();
    return 1;
  };
  if (met_size && !take(c->o_met, k.met_size == met_size ? &k.met : nullptr, met, met_size, &c->met)) return 0;
  c->o_f.resize(nfield);
  for (int j = 0; j < nfield; j++) {
    const bool kept = j < (int)k.f.size() && k.fsize[j] == field_size[j];
    if (!take(c->o_f[j], kept ? &k.f[j] : nullptr, fields[j], field_size[j], &c->fin[j])) return 0;
  }
  if (!carried.empty()) {
    // the rows to fetch from the host: one list for every carried array
    int *bc = c->carry_bc.as<int>();
    hipLaunchKernelGGL(k_cls_count, dim3((unsigned)ncls), dim3(kBlock), 0, s, (const uint8_t *)need, (long long)np, 1,
                       bc, (const int *)nullptr, 0);
    hipLaunchKernelGGL(k_scan_top, dim3(1), dim3(kBlock), 0, s, bc, (int)ncls, c->carry_cnt.as<int>(),
                       (const int *)nullptr, 0);
    hipLaunchKernelGGL(k_cls_scatter, dim3((unsigned)ncls), dim3(kBlock), 0, s, (const uint8_t *)need, (long long)np,
                       1, (const int *)bc, c->carry_ids.as<int>(), (const int *)nullptr, 0);
    HIPCK(c, hipGetLastError());
    int n = 0;
    HIPCK(c, hipMemcpyAsync(&n, c->carry_cnt.p, sizeof(int), hipMemcpyDeviceToHost, s));
    HIPCK(c, hipStreamSynchronize(s));
    std::vector<int> ids((size_t)n);
    if (n > 0) HIPCK(c, ctx_d2h(c, ids.data(), c->carry_ids.p, sizeof(int) * (size_t)n));
    for (const Arr &a : carried)
      if (!carry_host_rows(c, ids, a.host, a.row, a.dst->as<double>())) return 0;
  }
  if (c->cstream) HIPCK(c, hipStreamSynchronize(c->cstream));
  HIPCK(c, hipStreamSynchronize(s));
  k.valid = false; // its buffers now back the background (or were swapped out)
  carry_disarm(c);
  return 1;
}

// every way out of an armed set_solutions disarms the carry
static int carry_solutions(pmmg_hip_ctx *c, int met_size, const double *met, int nfield, const int *field_size,
                           const double *const *fields) {
  const int ok = carry_solutions_body(c, met_size, met, nfield, field_size, fields);
  carry_disarm(c);
  return ok;
}
