// pmmg_hip.hip — MI355X (gfx950) old->new mesh transfer: locate every new
// vertex in the background mesh and interpolate metric + fields (fp64).
//
// Replaces, behind the C-ABI of include/parmmg_hip.h, the per-group body of
// PMMG_interpMetricsAndFields (reference src/interpmesh_pmmg.c:477-741):
//   PMMG_locatePointVol      src/locate_pmmg.c:786-883     -> k_vol<layout> (fp32 filter walk + exact
//                                                             acceptance and continuation + interpolation)
//   PMMG_interp4bar_*        src/interpmesh_pmmg.c:206-270 -> vol_slot / vol_interp_packed in k_vol (pmmg_vol.hpp)
//   PMMG_locatePointBdy      src/locate_pmmg.c:587-723     -> k_bdy (locate + interpolate)  (pmmg_bdy.hpp)
//   exhaustive / closest     src/locate_pmmg.c:477-515, 737-770 -> k_exhaust_accept<NV>, k_exhaust_closest<NV>
//                                                             (pmmg_fallback.hpp)
//   PMMG_locate_setStart     src/locate_pmmg.c:931-986     -> k_start_tet / k_start_tri and the MAP variants of
//                                                             k_vol / k_bdy (USE_POINTMAP; pmmg_prep.hpp)
// Device arithmetic: pmmg_device.hpp; preparation and query order:
// pmmg_prep.hpp.
//
// Pipeline of one pmmg_hip_locate_interp (no host synchronisation inside):
//   main stream     reset, coherence test, frame, volume seeds | volume
//                   kernel (fp32 filter walk, exact acceptance and
//                   continuation, interpolation) | fallbacks | join
//   surface stream  the query order's lists (stable class compaction, or the
//                   Morton bins on a stream of their own), surface seeds,
//                   k_bdy, its fallbacks
// (the order is forced, or decided on the device by the coherence test and
// read back once by a large call: run_device)
//
// This file is the extern "C" entry points; the host side behind them is
// included here only, each part building on the one before:
#include "pmmg_ctx.hpp"    // the context, its buffers, error text, entry, switches
#include "pmmg_xfer.hpp"   // host-mode transfers and take_input
#include "pmmg_carry.hpp"  // the carry-over
#include "pmmg_call.hpp"   // one call on device pointers: Call, its stages, run_device, collect_stats
#include "pmmg_groups.hpp" // the groups call's lanes
#include "pmmg_comm.hpp"   // the RCCL loader and the all-gather
#include "pmmg_gather.hpp"
#include "pmmg_quality.hpp"

extern "C" {

int pmmg_hip_abi_version(void) { return PMMG_HIP_ABI_VERSION; }
int64_t pmmg_hip_stats_size(void) { return (int64_t)sizeof(pmmg_hip_stats); }
int64_t pmmg_hip_qual_histo_size(void) { return (int64_t)sizeof(pmmg_hip_qual_histo_t); }
int64_t pmmg_hip_len_histo_size(void) { return (int64_t)sizeof(pmmg_hip_len_histo_t); }

int pmmg_hip_device_count(void) {
  int n = 0;
  if (hipGetDeviceCount(&n) != hipSuccess) return 0;
  return n;
}

pmmg_hip_ctx *pmmg_hip_create(int device, int options) { return create_ctx(device, options); }

void pmmg_hip_destroy(pmmg_hip_ctx *c) {
  if (!c) return;
  delete c->lane_pool;
  for (pmmg_hip_ctx *l : c->lanes) pmmg_hip_destroy(l);
  (void)hipSetDevice(c->device);
  (void)snap_join(c);
  (void)hipStreamSynchronize(c->stream);
  (void)hipStreamSynchronize(c->stream2);
  if (c->stream3) (void)hipStreamSynchronize(c->stream3);
  if (c->stream_f) (void)hipStreamSynchronize(c->stream_f);
  if (c->cstream) (void)hipStreamSynchronize(c->cstream);
  // every stream is idle and still exists: the device buffers go now, before the streams
  *static_cast<CtxBufs *>(c) = CtxBufs{};
  for (int i = 0; i < EV_COUNT; i++)
    if (c->ev[i]) (void)hipEventDestroy(c->ev[i]);
  for (int b = 0; b < 2; b++) {
    if (c->stage[b]) (void)hipHostFree(c->stage[b]);
    if (c->stage_ev[b]) (void)hipEventDestroy(c->stage_ev[b]);
  }
  delete c->pool;
  if (c->comm && c->comm_owned && rccl().ok) (void)rccl().commDestroy(c->comm);
  if (!c->borrowed_streams) {
    if (c->stream2 && c->stream2 != c->stream) (void)hipStreamDestroy(c->stream2);
    if (c->stream) (void)hipStreamDestroy(c->stream);
  }
  if (c->stream3) (void)hipStreamDestroy(c->stream3);
  if (c->stream_f) (void)hipStreamDestroy(c->stream_f);
  if (c->flag_host) (void)hipHostFree(c->flag_host);
  if (c->cstream) (void)hipStreamDestroy(c->cstream);
  delete c;
}

const char *pmmg_hip_last_error(pmmg_hip_ctx *c) { return c ? c->err : "null context"; }

// shared body of the two background entry points: tet8 != NULL selects the
// packed {v[4], adja[4]} records, else the separate tetv / adja arrays.
// adja == NULL: the adjacency is built on the device (MMG3D_hashTetra's
// result, into owned tet8 records); triv == NULL with nt < 0: the boundary
// trias and their adjacency are built on the device (MMG5_chkBdryTria +
// MMG3D_hashTria for an old mesh without input trias); adjt == NULL with
// triv given: the tria adjacency is built on the device.
static int set_background_impl(pmmg_hip_ctx *c, int np, const double *xyz, int ne, const int *tetv, const int *adja,
                               const int *tet8, int nt, const int *triv, const int *adjt, double hausd, int where) {
  if (!enter(c)) return 0;
  c->start_valid = false; // (the start tables belong to the background they were built on)
  const bool packed = tet8 != nullptr;
  const bool build_bdy = nt < 0 && !triv;
  if (np <= 0 || ne <= 0 || !xyz || (!packed && !tetv) || (nt < 0 && triv) || (nt > 0 && !triv)) {
    set_err(c, "set_background: invalid arguments (np=%d ne=%d nt=%d)", np, ne, nt);
    return 0;
  }
  if (ne >= kTetMax) {
    set_err(c, "set_background: %d tetra exceed the 4*k+i adjacency encoding (2^29)", ne);
    return 0;
  }
  const bool dev = where == PMMG_HIP_DEVICE;
  if (dev) {
    const void *t0 = packed ? (const void *)tet8 : (const void *)tetv;
    if (!aligned<16>(t0) || (!packed && !aligned<16>(adja))) {
      set_err(c, "set_background: device tetra arrays must be 16-byte aligned");
      return 0;
    }
  }
  c->bg.np = np;
  c->bg.ne = ne;
  c->bg.hausd = hausd;
  // vertices
  if (c->carry_slot >= 0 && dev) {
    set_err(c, "set_background: a carry-over is armed; it takes host-mode (PMMG_HIP_HOST) calls");
    carry_disarm(c);
    return 0;
  }
  if (c->carry_slot >= 0) {
    if (!carry_vertices(c, np, xyz)) return 0;
    c->bg.xyz = c->o_xyz.as<const double>();
  } else if (!take_input(c, where, xyz, sizeof(double) * 3 * (size_t)np, c->o_xyz, &c->bg.xyz)) {
    return 0;
  }
  // tetra
  const size_t row4 = sizeof(int) * 4 * (size_t)ne;
  const int *d_tetv = nullptr; // input of the device adjacency
  if (packed) {
    if (!take_input(c, where, tet8, 2 * row4, c->o_tetv, &c->bg.tetv)) return 0;
    c->bg.adja = c->bg.tetv + 1;
    c->bg.tstride = 2;
  } else if (adja) {
    if (!take_input(c, where, tetv, row4, c->o_tetv, &c->bg.tetv) ||
        !take_input(c, where, adja, row4, c->o_adja, &c->bg.adja))
      return 0;
    c->bg.tstride = 1;
  } else { // device adjacency into owned tet8 records
    if (!take_input(c, where, tetv, row4, c->o_tet4, &d_tetv) || !ensure(c, c->o_tetv, 2 * row4)) return 0;
    c->bg.tetv = c->o_tetv.as<const int4>();
    c->bg.adja = c->bg.tetv + 1;
    c->bg.tstride = 2;
  }
  // boundary trias handed over
  if (!build_bdy) {
    const size_t row3 = sizeof(int) * 3 * (size_t)nt;
    if (!take_input(c, where, triv, row3, c->o_triv, &c->bg.triv)) return 0;
    c->bg.adjt = nullptr;
    if (adjt && !take_input(c, where, adjt, row3, c->o_adjt, &c->bg.adjt)) return 0;
    c->bg.nt = nt;
  }
  const bool tria_adj = !build_bdy && nt > 0 && !adjt;
  // the device snapshot (PMMG_create_oldGrp's arrays): adjacency, boundary
  // trias, tria adjacency, each on the context stream
  auto snapshot = [c, np, ne, d_tetv, build_bdy, tria_adj]() -> int {
    if (d_tetv && !pmmg_snap_adjacency(c->stream, np, ne, d_tetv, nullptr, c->o_tetv.as<int>(), &c->snap_cache, c->err,
                                     sizeof(c->err))) {
      fprintf(stderr, "[parmmg_hip] %s\n", c->err);
      return 0;
    }
    if (build_bdy) {
      const TetView m{ne, reinterpret_cast<const int *>(c->bg.tetv), c->bg.tstride,
                      reinterpret_cast<const int *>(c->bg.adja), c->bg.tstride};
      int cnt = 0, ntb = 0;
      char msg[256];
      pmmg_snap_boundary(c->stream, np, m, nullptr, 0, &cnt, nullptr, nullptr, &c->snap_cache, msg,
                         sizeof(msg)); // counts (fails on capacity 0 when there are trias)
      if (!ensure(c, c->o_triv, sizeof(int) * 3 * (size_t)cnt) || !ensure(c, c->o_adjt, sizeof(int) * 3 * (size_t)cnt))
        return 0;
      if (!pmmg_snap_boundary(c->stream, np, m, nullptr, cnt, &ntb, c->o_triv.as<int>(), c->o_adjt.as<int>(),
                              &c->snap_cache, c->err, sizeof(c->err))) {
        fprintf(stderr, "[parmmg_hip] %s\n", c->err);
        return 0;
      }
      c->bg.triv = c->o_triv.as<const int>();
      c->bg.adjt = c->o_adjt.as<const int>();
      c->bg.nt = ntb;
    }
    if (tria_adj) {
      if (!ensure(c, c->o_adjt, sizeof(int) * 3 * (size_t)c->bg.nt)) return 0;
      if (!pmmg_snap_tria_adjacency(c->stream, np, c->bg.nt, c->bg.triv, c->o_adjt.as<int>(), &c->snap_cache, c->err,
                                    sizeof(c->err))) {
        fprintf(stderr, "[parmmg_hip] %s\n", c->err);
        return 0;
      }
      c->bg.adjt = c->o_adjt.as<const int>();
    }
    return 1;
  };
  if (!dev && (d_tetv || build_bdy || tria_adj)) {
    // host mode: the snapshot runs in a host thread (its kernels on the
    // context stream) while the caller goes on to set_solutions, whose
    // uploads use the copy stream; the next other call joins it
    c->snap_ok = 1;
    c->snap = std::thread([c, snapshot] {
      c->snap_ok = hipSetDevice(c->device) == hipSuccess ? snapshot() : 0;
    });
    return 1;
  }
  if (!snapshot()) {
    invalidate_bg(c);
    return 0;
  }
  if (!dev) HIPCK(c, hipStreamSynchronize(c->stream));
  return 1;
}

int pmmg_hip_set_background(pmmg_hip_ctx *c, int np, const double *xyz, int ne, const int *tetv, const int *adja,
                            int nt, const int *triv, const int *adjt, double hausd, int where) {
  if (c && !tetv) {
    set_err(c, "set_background: tetv is NULL");
    return 0;
  }
  return set_background_impl(c, np, xyz, ne, tetv, adja, nullptr, nt, triv, adjt, hausd, where);
}

int pmmg_hip_set_background_tet8(pmmg_hip_ctx *c, int np, const double *xyz, int ne, const int *tet8, int nt,
                                 const int *triv, const int *adjt, double hausd, int where) {
  if (c && !tet8) {
    set_err(c, "set_background_tet8: tet8 is NULL");
    return 0;
  }
  return set_background_impl(c, np, xyz, ne, nullptr, nullptr, tet8, nt, triv, adjt, hausd, where);
}

int pmmg_hip_set_solutions(pmmg_hip_ctx *c, int met_size, const double *met, int nfield, const int *field_size,
                           const double *const *fields, int where) {
  if (!c) return 0;
  HIPCK(c, hipSetDevice(c->device));
  if (!valid_met_size(met_size)) {
    set_err(c, "set_solutions: metric size %d (expected 0, 1 or 6)", met_size);
    return 0;
  }
  if (nfield < 0 || nfield + (met_size ? 1 : 0) > kMaxSlot) {
    set_err(c, "set_solutions: %d fields exceed the %d-slot limit", nfield, kMaxSlot);
    return 0;
  }
  if (met_size && !met) {
    set_err(c, "set_solutions: metric pointer is NULL");
    return 0;
  }
  for (int j = 0; j < nfield; j++) {
    // MMG5_Scalar / MMG5_Vector / MMG5_Tensor are the only solution types at vertices
    if (!fields || !fields[j] || !valid_field_size(field_size[j])) {
      set_err(c, "set_solutions: field %d has size %d (expected 1, 3 or 6)", j, field_size ? field_size[j] : -1);
      return 0;
    }
    if (where == PMMG_HIP_DEVICE && field_size[j] == 6 && ((uintptr_t)fields[j] & 15)) {
      set_err(c, "set_solutions: device tensor field %d must be 16-byte aligned", j);
      return 0;
    }
  }
  if (where == PMMG_HIP_DEVICE && met_size == 6 && ((uintptr_t)met & 15)) {
    set_err(c, "set_solutions: a device tensor metric must be 16-byte aligned");
    return 0;
  }
  size_t np = (size_t)c->bg.np;
  if (np == 0) {
    set_err(c, "set_solutions: call pmmg_hip_set_background first");
    return 0;
  }
  c->met_size = met_size;
  c->nfield = nfield;
  c->fsize.assign(field_size, field_size + nfield);
  c->fin.resize(nfield);
  c->rec = nullptr;
  c->rstride = 0;
  const bool dev = where == PMMG_HIP_DEVICE;
  if (dev && c->carry_slot >= 0) {
    set_err(c, "set_solutions: a carry-over is armed; it takes host-mode (PMMG_HIP_HOST) calls");
    carry_disarm(c);
    return 0;
  }
  if (c->carry_slot >= 0) return carry_solutions(c, met_size, met, nfield, field_size, fields);
  // host mode: through the copy stream (beside a deferred snapshot)
  if (!dev && !copy_stream(c)) return 0;
  if ((dev || met_size) && !take_input(c, where, met, sizeof(double) * met_size * np, c->o_met, &c->met, c->cstream))
    return 0;
  DevBuf none; // (device mode owns no copy)
  if (!dev) c->o_f.resize(nfield);
  for (int j = 0; j < nfield; j++)
    if (!take_input(c, where, fields[j], sizeof(double) * field_size[j] * np, dev ? none : c->o_f[j], &c->fin[j],
                    c->cstream))
      return 0;
  if (!dev) HIPCK(c, hipStreamSynchronize(c->cstream));
  return 1;
}

int pmmg_hip_set_solutions_packed(pmmg_hip_ctx *c, int met_size, int nfield, const int *field_size,
                                  const double *rec, int where) {
  if (!c) return 0;
  HIPCK(c, hipSetDevice(c->device));
  if (!valid_met_size(met_size) || nfield < 0 || nfield + (met_size ? 1 : 0) > kMaxSlot ||
      (nfield > 0 && !field_size) || !rec) {
    set_err(c, "set_solutions_packed: invalid arguments (met_size=%d nfield=%d)", met_size, nfield);
    return 0;
  }
  int K = met_size;
  for (int j = 0; j < nfield; j++) {
    if (!valid_field_size(field_size[j])) {
      set_err(c, "set_solutions_packed: field %d has size %d (expected 1, 3 or 6)", j, field_size[j]);
      return 0;
    }
    K += field_size[j];
  }
  if (K == 0 || !packed_supported(met_size, nfield, field_size)) {
    set_err(c, "set_solutions_packed: slot layout not supported by the packed records (at most 16 doubles, a "
               "compiled layout); use pmmg_hip_set_solutions");
    return 0;
  }
  if (where == PMMG_HIP_DEVICE && ((uintptr_t)rec & 15)) {
    set_err(c, "set_solutions_packed: device records must be 16-byte aligned");
    return 0;
  }
  const size_t np = (size_t)c->bg.np;
  if (np == 0) {
    set_err(c, "set_solutions_packed: call pmmg_hip_set_background first");
    return 0;
  }
  if (c->carry_slot >= 0) {
    set_err(c, "set_solutions_packed: a carry-over is armed; it takes pmmg_hip_set_solutions (the kept rows are "
               "per-solution arrays)");
    carry_disarm(c);
    return 0;
  }
  c->met_size = met_size;
  c->nfield = nfield;
  c->fsize.assign(field_size, field_size + nfield);
  c->fin.assign(nfield, nullptr);
  c->met = nullptr;
  c->rstride = (K + 1) & ~1;
  const bool dev = where == PMMG_HIP_DEVICE;
  if (!dev && !copy_stream(c)) return 0;
  if (!take_input(c, where, rec, sizeof(double) * c->rstride * np, c->o_rec, &c->rec, c->cstream)) return 0;
  if (!dev) HIPCK(c, hipStreamSynchronize(c->cstream));
  return 1;
}

int pmmg_hip_sync(pmmg_hip_ctx *c, pmmg_hip_stats *stats) {
  if (!enter(c)) return 0;
  for (pmmg_hip_ctx *l : c->lanes)
    if (hipStreamSynchronize(l->stream) != hipSuccess) {
      set_err(c, "sync: group lane failed: %s", l->err);
      return 0;
    }
  HIPCK(c, hipStreamSynchronize(c->stream));
  if (stats && c->pending) return collect_stats(c, stats);
  return 1;
}

// The armed point map, taken by a locate_interp(_rec) call whatever becomes
// of the call; 0 (with the map dropped) when it was armed for another np_new.
static int take_point_map(pmmg_hip_ctx *c, int np_new, const int **src) {
  *src = c->map_src;
  c->map_src = nullptr;
  if (*src && c->map_np != np_new) {
    set_err(c, "locate_interp: the point map was armed for %d new points, the call has %d", c->map_np, np_new);
    return 0;
  }
  return 1;
}

int pmmg_hip_set_point_map(pmmg_hip_ctx *c, int np_new, const int *src, int where) {
  if (!c) return 0;
  c->map_src = nullptr;
  if (np_new <= 0 || !src) {
    set_err(c, "set_point_map: np_new = %d or src NULL", np_new);
    return 0;
  }
  if (where != PMMG_HIP_DEVICE && !enter(c)) return 0; // (the copy of a host map goes through the device)
  if (!take_input(c, where, src, sizeof(int) * (size_t)np_new, c->map_own, &c->map_src)) return 0;
  c->map_np = np_new;
  return 1;
}

int pmmg_hip_start_elements(pmmg_hip_ctx *c, int *start_tet, int *start_tri, int where) {
  if (!enter(c)) return 0;
  if (c->bg.ne <= 0) {
    set_err(c, "start_elements: no background set");
    return 0;
  }
  if (!start_tables(c)) return 0;
  const size_t bytes = sizeof(int) * (size_t)c->bg.np;
  const int *tab = c->start_tab.as<const int>();
  const hipMemcpyKind kind = where == PMMG_HIP_DEVICE ? hipMemcpyDeviceToDevice : hipMemcpyDeviceToHost;
  if (start_tet) HIPCK(c, hipMemcpyAsync(start_tet, tab, bytes, kind, c->stream));
  if (start_tri) HIPCK(c, hipMemcpyAsync(start_tri, tab + c->bg.np, bytes, kind, c->stream));
  HIPCK(c, hipStreamSynchronize(c->stream));
  return 1;
}

int pmmg_hip_locate_interp(pmmg_hip_ctx *c, int np_new, const double *xyz_new, const uint8_t *pclass,
                           double *met_out, double *const *fields_out, int *elem_out, int8_t *hit_out,
                           pmmg_hip_stats *stats, int where) {
  if (!c) return 0;
  const int *map_src = nullptr;
  if (!take_point_map(c, np_new, &map_src)) return 0;
  if (!enter(c)) return 0;
  if (c->bg.ne <= 0) {
    set_err(c, "locate_interp: no background set");
    return 0;
  }
  if (np_new <= 0) {
    if (stats) memset(stats, 0, sizeof(*stats));
    return 1;
  }
  if (!xyz_new || !pclass) {
    set_err(c, "locate_interp: xyz_new / pclass is NULL");
    return 0;
  }
  if (where == PMMG_HIP_DEVICE) {
    if (((uintptr_t)met_out & 15) && c->met_size == 6) {
      set_err(c, "locate_interp: a device tensor output must be 16-byte aligned");
      return 0;
    }
    if (!run_device(c, np_new, xyz_new, pclass, met_out, fields_out, elem_out, hit_out, nullptr, map_src)) return 0;
    if (stats) return pmmg_hip_sync(c, stats);
    return 1;
  }
  // host mode: queries in, outputs out through the pinned staging buffers.
  // The device output rows start as a sentinel NaN, and only the rows the
  // step wrote (sentinel gone; elem / hit where hit != 0) are copied back, so
  // the caller's other rows stay untouched without being uploaded.
  size_t n = (size_t)np_new;
  const double t0 = now_s();
  if (!upload(c, c->h_xyz, xyz_new, sizeof(double) * 3 * n)) return 0;
  if (!upload(c, c->h_cls, pclass, n)) return 0;
  double *dmet = nullptr;
  auto sentinel_fill = [&](DevBuf &b, size_t ndbl) -> int {
    if (!ensure(c, b, sizeof(double) * ndbl)) return 0;
    hipLaunchKernelGGL(k_fill64, dim3(blocks_for((long long)ndbl, 4096)), dim3(kBlock), 0, c->stream,
                       b.as<unsigned long long>(), (long long)ndbl, kSentinel);
    return 1;
  };
  if (c->met_size) {
    if (!met_out) {
      set_err(c, "locate_interp: met_out is NULL");
      return 0;
    }
    if (!sentinel_fill(c->h_met, (size_t)c->met_size * n)) return 0;
    dmet = c->h_met.as<double>();
  }
  c->h_f.resize(c->nfield);
  std::vector<double *> dfields(c->nfield > 0 ? c->nfield : 1, nullptr);
  for (int j = 0; j < c->nfield; j++) {
    if (!fields_out || !fields_out[j]) {
      set_err(c, "locate_interp: fields_out[%d] is NULL", j);
      return 0;
    }
    if (!sentinel_fill(c->h_f[j], (size_t)c->fsize[j] * n)) return 0;
    dfields[j] = c->h_f[j].as<double>();
  }
  if (!ensure(c, c->h_elem, sizeof(int) * n) || !ensure(c, c->h_hit, n)) return 0;
  HIPCK(c, hipMemsetAsync(c->h_hit.p, 0, n, c->stream));
  if (!run_device(c, np_new, c->h_xyz.as<const double>(), c->h_cls.as<const uint8_t>(), dmet, dfields.data(),
                  c->h_elem.as<int>(), c->h_hit.as<int8_t>(), nullptr, map_src))
    return 0;
  const double t1 = now_s();
  std::vector<int8_t> hh(n);
  if (!d2h_rows(c, hh.data(), c->h_hit.p, n, 1, AllRows{})) return 0;
  const double t2 = now_s();
  auto written = [&](size_t, const char *row) {
    unsigned long long u;
    memcpy(&u, row, 8);
    return u != kSentinel;
  };
  auto processed = [&](size_t r, const char *) { return hh[r] != 0; };
  if (dmet && !d2h_rows(c, met_out, dmet, n, sizeof(double) * c->met_size, written)) return 0;
  for (int j = 0; j < c->nfield; j++)
    if (!d2h_rows(c, fields_out[j], dfields[j], n, sizeof(double) * c->fsize[j], written)) return 0;
  if (elem_out && !d2h_rows(c, elem_out, c->h_elem.p, n, sizeof(int), processed)) return 0;
  if (hit_out)
    c->pool->run(n, n >= 65536 ? c->pool->th.size() + 1 : 1, [&](size_t a, size_t e) {
      for (size_t r = a; r < e; r++)
        if (hh[r]) hit_out[r] = hh[r];
    });
  if (c->verbose)
    fprintf(stderr, "[parmmg_hip] host locate: uploads + enqueue %.2f ms, step + hit codes %.2f ms, rows %.2f ms\n",
            1e3 * (t1 - t0), 1e3 * (t2 - t1), 1e3 * (now_s() - t2));
  c->last_host_np = np_new; // what pmmg_hip_keep can keep
  c->last_host_met = c->met_size;
  c->last_host_fsize = c->fsize;
  if (stats) return collect_stats(c, stats);
  return 1;
}

int pmmg_hip_locate_interp_rec(pmmg_hip_ctx *c, int np_new, const double *xyz_new, const uint8_t *pclass,
                               double *rec_out, int *elem_out, int8_t *hit_out, pmmg_hip_stats *stats, int where) {
  if (!c) return 0;
  const int *map_src = nullptr;
  if (!take_point_map(c, np_new, &map_src)) return 0;
  if (!enter(c)) return 0;
  if (where != PMMG_HIP_DEVICE) {
    set_err(c, "locate_interp_rec: device pointers only (PMMG_HIP_DEVICE)");
    return 0;
  }
  if (c->bg.ne <= 0) {
    set_err(c, "locate_interp_rec: no background set");
    return 0;
  }
  if (!c->rec) {
    set_err(c, "locate_interp_rec: output records need packed input records (pmmg_hip_set_solutions_packed)");
    return 0;
  }
  if (np_new <= 0) {
    if (stats) memset(stats, 0, sizeof(*stats));
    return 1;
  }
  if (!xyz_new || !pclass || !rec_out || ((uintptr_t)rec_out & 15)) {
    set_err(c, "locate_interp_rec: xyz_new / pclass / rec_out NULL or rec_out not 16-byte aligned");
    return 0;
  }
  if (!run_device(c, np_new, xyz_new, pclass, nullptr, nullptr, elem_out, hit_out, rec_out, map_src)) return 0;
  if (stats) return pmmg_hip_sync(c, stats);
  return 1;
}

// ---- carry-over entry points (see "carry-over" above)

int pmmg_hip_keep(pmmg_hip_ctx *c, int slot) {
  if (!c) return 0;
  if (slot < 0 || slot >= 1024) {
    set_err(c, "keep: slot %d out of [0, 1024)", slot);
    return 0;
  }
  if (c->last_host_np <= 0) {
    set_err(c, "keep: no host-mode pmmg_hip_locate_interp to keep since the last keep");
    return 0;
  }
  if ((int)c->kept.size() <= slot) c->kept.resize(slot + 1);
  pmmg_hip_ctx::Kept &k = c->kept[slot];
  std::swap(k.xyz, c->h_xyz);
  k.met_size = c->last_host_met;
  if (k.met_size) std::swap(k.met, c->h_met);
  k.fsize = c->last_host_fsize;
  k.f.resize(k.fsize.size());
  for (size_t j = 0; j < k.f.size(); j++) std::swap(k.f[j], c->h_f[j]);
  k.np = c->last_host_np;
  k.valid = true;
  c->last_host_np = 0;
  return 1;
}

int pmmg_hip_carry_over(pmmg_hip_ctx *c, int slot, int np, const int *src) {
  if (!c) return 0;
  if (np == 0) { // drop the slot and free its device buffers
    if (c->carry_slot == slot && c->carry_bg) {
      set_err(c, "carry_over: slot %d is being carried (set_background took it, set_solutions has not run)", slot);
      return 0;
    }
    if (slot >= 0 && slot < (int)c->kept.size()) {
      pmmg_hip_ctx::Kept &k = c->kept[slot];
      if (!enter(c)) return 0;
      HIPCK(c, hipStreamSynchronize(c->stream));
      k = pmmg_hip_ctx::Kept{};
    }
    if (c->carry_slot == slot) carry_disarm(c);
    return 1;
  }
  if (slot < 0 || slot >= (int)c->kept.size() || !c->kept[slot].valid) {
    set_err(c, "carry_over: slot %d holds nothing (pmmg_hip_keep after a host-mode call)", slot);
    return 0;
  }
  const pmmg_hip_ctx::Kept &k = c->kept[slot];
  if (np <= 0 || (!src && np != k.np)) {
    set_err(c, "carry_over: %d vertices for %d kept points without a map", np, k.np);
    return 0;
  }
  c->carry_src.clear();
  if (src) {
    for (int i = 0; i < np; i++)
      if (src[i] < 0 || src[i] > k.np) {
        set_err(c, "carry_over: src[%d] = %d out of [0, %d]", i, src[i], k.np);
        return 0;
      }
    c->carry_src.assign(src, src + np);
  }
  c->carry_slot = slot;
  c->carry_np = np;
  c->carry_bg = false;
  return 1;
}

int pmmg_hip_release_scratch(pmmg_hip_ctx *c) {
  if (!enter(c)) return 0;
  HIPCK(c, hipStreamSynchronize(c->stream));
  HIPCK(c, hipStreamSynchronize(c->stream2));
  if (c->stream3) HIPCK(c, hipStreamSynchronize(c->stream3));
  c->snap_cache = SnapCache{};
  c->stats_cache = StatsCache{};
  c->graph_cache = GraphCache{};
  c->contig_cache = ContigCache{};
  c->split_cache = SplitCache{};
  c->move_cache = MoveCache{};
  c->merge_cache = MergeCache{};
  for (DevBuf *b : {&c->bvals2, &c->rs_hist, &c->rs_csum, &c->start_tab}) b->release();
  c->start_valid = false; // (the next call with a point map builds the start tables again)
  for (pmmg_hip_ctx *l : c->lanes) pmmg_hip_destroy(l);
  c->lanes.clear();
  return 1;
}

int64_t pmmg_hip_bytes_up(pmmg_hip_ctx *c, int reset) {
  if (!c) return -1;
  const int64_t b = c->bytes_up;
  if (reset) c->bytes_up = 0;
  return b;
}

int pmmg_hip_locate_interp_groups(pmmg_hip_ctx *c, int ngroup, const pmmg_hip_group *groups,
                                  pmmg_hip_stats *stats) {
  return c ? groups_call(c, ngroup, groups, stats) : 0;
}

// ---- background snapshot (pmmg_snapshot.hip)

int pmmg_hip_build_adjacency(pmmg_hip_ctx *c, int np, int ne, const int *tetv, int *adja, int *tet8) {
  if (!enter(c)) return 0;
  if (np <= 0 || ne <= 0 || !tetv || (!adja && !tet8)) {
    set_err(c, "build_adjacency: invalid arguments (np=%d ne=%d)", np, ne);
    return 0;
  }
  if (ne >= kTetMax) {
    set_err(c, "build_adjacency: %d tetra exceed the 4*k+i adjacency encoding (2^29)", ne);
    return 0;
  }
  if (!aligned<16>(tetv) || (adja && !aligned<16>(adja)) || (tet8 && !aligned<16>(tet8))) {
    set_err(c, "build_adjacency: device arrays must be 16-byte aligned");
    return 0;
  }
  return pmmg_snap_adjacency(c->stream, np, ne, tetv, adja, tet8, &c->snap_cache, c->err, sizeof(c->err));
}

int pmmg_hip_tetra_qual(pmmg_hip_ctx *c, int np, const double *xyz, int ne, const int *tetv, int met_size,
                        const double *met, double *qual, double *minqual) {
  if (!enter(c)) return 0;
  if (np < 0 || ne < 0 || (ne > 0 && (!xyz || !tetv || !qual)) || !minqual ||
      (met_size == 6 && ne > 0 && !met) || !valid_met_size(met_size)) {
    set_err(c, "tetra_qual: invalid arguments (np=%d ne=%d met_size=%d)", np, ne, met_size);
    return 0;
  }
  if (ne > 0 && !aligned<16>(tetv)) {
    set_err(c, "tetra_qual: tetv must be 16-byte aligned");
    return 0;
  }
  if (!ensure(c, c->qmin, sizeof(unsigned long long))) return 0;
  unsigned long long bits = 0;
  if (!pmmg_qual_tetra(c->stream, np, xyz, ne, tetv, met_size, met, qual, c->qmin.as<unsigned long long>(), &bits)) {
    set_err(c, "tetra_qual: kernel launch or copy failed");
    return 0;
  }
  // MMG3D_tetraQual: minqual starts at 2/ALPHAD, returns ALPHAD * minqual
  const double alphad = 20.7846096908265; // MMG3D_ALPHAD = 12 sqrt(3): a regular tetra has quality 1
  double mn = 2.0 / alphad;
  if (bits != ~0ULL) {
    double q;
    memcpy(&q, &bits, sizeof q);
    if (q < mn) mn = q;
  }
  *minqual = alphad * mn;
  return 1;
}

int pmmg_hip_qual_histo(pmmg_hip_ctx *c, int ne, const int *tetv, const double *qual, pmmg_hip_qual_histo_t *out) {
  if (!enter(c)) return 0;
  if (ne < 0 || (ne > 0 && (!tetv || !qual)) || !out) {
    set_err(c, "qual_histo: invalid arguments (ne=%d)", ne);
    return 0;
  }
  if (ne > 0 && !aligned<16>(tetv)) {
    set_err(c, "qual_histo: tetv must be 16-byte aligned");
    return 0;
  }
  return pmmg_stats_qual_histo(c->stream, ne, tetv, qual, out, &c->stats_cache, c->err, sizeof(c->err));
}

int pmmg_hip_edge_lengths(pmmg_hip_ctx *c, int np, const double *xyz, int ne, const int *tetv, int met_size,
                          const double *met, int nskip, const int *skip, pmmg_hip_len_histo_t *out, int cap,
                          int *edge_out, double *len_out) {
  if (!enter(c)) return 0;
  if (met_size != 1 && met_size != 6) {
    set_err(c, "edge_lengths: met_size %d (an edge length needs an iso (1) or aniso (6) metric)", met_size);
    return 0;
  }
  if (np < 0 || ne < 0 || (ne > 0 && (np < 1 || !xyz || !tetv || !met)) || nskip < 0 || (nskip > 0 && !skip) || !out ||
      cap < 0) {
    set_err(c, "edge_lengths: invalid arguments (np=%d ne=%d nskip=%d cap=%d)", np, ne, nskip, cap);
    return 0;
  }
  if ((ne > 0 && !aligned<16>(tetv)) || !aligned<8>(skip) || !aligned<8>(edge_out) || !aligned<8>(len_out)) {
    set_err(c, "edge_lengths: tetv must be 16-byte, skip / edge_out / len_out 8-byte aligned");
    return 0;
  }
  return pmmg_stats_edge_lengths(c->stream, np, xyz, ne, tetv, met_size, met, nskip, skip, out, cap, edge_out, len_out,
                                 c->edge_hash, &c->stats_cache, c->err, sizeof(c->err));
}

int64_t pmmg_hip_mesh_stats_bytes(pmmg_hip_ctx *c) { return c ? pmmg_stats_cache_bytes(&c->stats_cache) : -1; }

int pmmg_hip_compute_wgt_mesh(pmmg_hip_ctx *c, int np, const double *xyz, int ne, const int *tetv, const int *xt,
                              const uint16_t *ftag, int met_size, const double *met, int tag, double *qual) {
  if (!enter(c)) return 0;
  if (np < 0 || ne < 0 || (ne > 0 && (!xyz || !tetv || !xt || !ftag || !qual)) ||
      !valid_met_size(met_size) || (met_size && ne > 0 && !met)) {
    set_err(c, "compute_wgt_mesh: invalid arguments (np=%d ne=%d met_size=%d)", np, ne, met_size);
    return 0;
  }
  if (ne > 0 && (!aligned<16>(tetv) || !aligned<8>(ftag))) {
    set_err(c, "compute_wgt_mesh: tetv must be 16-byte and ftag 8-byte aligned");
    return 0;
  }
  if (!pmmg_wgt_mesh(c->stream, xyz, ne, tetv, xt, ftag, met_size, met, tag, qual)) {
    set_err(c, "compute_wgt_mesh: kernel launch failed");
    return 0;
  }
  return 1;
}

int pmmg_hip_compute_wgt_faces(pmmg_hip_ctx *c, int np, const double *xyz, const int *tetv, int nface,
                               const int *face, int met_size, const double *met, double *wgt) {
  if (!enter(c)) return 0;
  if (np < 0 || nface < 0 || (nface > 0 && (!xyz || !tetv || !face || !wgt)) ||
      !valid_met_size(met_size) || (met_size && nface > 0 && !met)) {
    set_err(c, "compute_wgt_faces: invalid arguments (np=%d nface=%d met_size=%d)", np, nface, met_size);
    return 0;
  }
  if (nface > 0 && (!aligned<16>(tetv) || !aligned<8>(face))) {
    set_err(c, "compute_wgt_faces: tetv must be 16-byte and face 8-byte aligned");
    return 0;
  }
  if (!pmmg_wgt_faces(c->stream, xyz, tetv, nface, face, met_size, met, wgt)) {
    set_err(c, "compute_wgt_faces: kernel launch failed");
    return 0;
  }
  return 1;
}

int pmmg_hip_metis_graph(pmmg_hip_ctx *c, int np, const double *xyz, int ne, const int *tetv, const int *adja,
                         const int *tet8, int met_size, const double *met, int cap, int64_t *nadjncy, int *xadj,
                         int *adjncy, int *adjwgt) {
  if (!enter(c)) return 0;
  const bool wgt = adjwgt != nullptr;
  TetView m;
  const TetArgs ta = tet_view(ne, tetv, adja, tet8, wgt ? TET_NEED_TETV : 0, &m);
  if (np < 0 || ne < 0 || !nadjncy || !xadj || cap < 0 || (cap > 0 && !adjncy) || ta == TET_MISSING ||
      (wgt && ne > 0 && (np < 1 || !xyz || !valid_met_size(met_size) || (met_size && !met)))) {
    set_err(c, "metis_graph: invalid arguments (np=%d ne=%d met_size=%d cap=%d)", np, ne, met_size, cap);
    return 0;
  }
  if (ta == TET_TOOMANY) {
    set_err(c, "metis_graph: %d tetra exceed the 4*k+i adjacency encoding (2^29)", ne);
    return 0;
  }
  if (ta == TET_MISALIGNED || (ne > 0 && wgt && (!aligned<8>(xyz) || !aligned<8>(met)))) {
    set_err(c, "metis_graph: device tetra arrays must be 16-byte, xyz / met 8-byte aligned");
    return 0;
  }
  if (!aligned<4>(xadj) || !aligned<4>(adjncy) || !aligned<4>(adjwgt)) {
    set_err(c, "metis_graph: xadj / adjncy / adjwgt must be 4-byte aligned");
    return 0;
  }
  if (ne > 0 && !m.adja && np < 1) {
    set_err(c, "metis_graph: invalid arguments (np=%d: the adjacency is built from tetv)", np);
    return 0;
  }
  return pmmg_graph_metis(c->stream, np, xyz, m, wgt ? 1 : 0, met_size, met, cap, nadjncy, xadj, adjncy, adjwgt,
                          &c->graph_cache, &c->snap_cache, c->err, sizeof(c->err));
}

// ---- contiguity of a partition (pmmg_contig.hip)

// the arguments the two contiguity calls share; fills *m
static int contig_args(pmmg_hip_ctx *c, const char *who, int ne, const int *tetv, const int *adja, const int *tet8,
                       const int *part, int ncolor, TetView *m) {
  const TetArgs ta = tet_view(ne, tetv, adja, tet8, 0, m);
  if (ne < 0 || ncolor < 1 || ta == TET_MISSING) {
    set_err(c, "%s: invalid arguments (ne=%d ncolor=%d)", who, ne, ncolor);
    return 0;
  }
  if (!part && ncolor != 1) {
    set_err(c, "%s: part == NULL is one colour for the whole mesh: ncolor = %d must be 1", who, ncolor);
    return 0;
  }
  if (ta == TET_TOOMANY) {
    set_err(c, "%s: %d tetra exceed the 4*k+i adjacency encoding (2^29)", who, ne);
    return 0;
  }
  if (ta == TET_MISALIGNED || (ne > 0 && !aligned<4>(part))) {
    set_err(c, "%s: device tetra arrays must be 16-byte, part 4-byte aligned", who);
    return 0;
  }
  return 1;
}

int pmmg_hip_part_subgroups(pmmg_hip_ctx *c, int ne, const int *tetv, const int *adja, const int *tet8,
                            const int *part, int ncolor, int *head, int *flag, int *ncomp, int cap,
                            pmmg_hip_subgroup *sub, int64_t *nsub, int *rounds) {
  if (!enter(c)) return 0;
  TetView m;
  if (!contig_args(c, "part_subgroups", ne, tetv, adja, tet8, part, ncolor, &m)) return 0;
  if (!ncomp || !nsub || cap < 0 || (cap > 0 && !sub) || !aligned<4>(head) || !aligned<4>(flag)) {
    set_err(c, "part_subgroups: invalid arguments (cap=%d; head / flag must be 4-byte aligned)", cap);
    return 0;
  }
  return pmmg_contig_subgroups(c->stream, m, part, ncolor, head, flag, ncomp, cap, sub, nsub, rounds,
                               &c->contig_cache, &c->snap_cache, c->err, sizeof(c->err));
}

int pmmg_hip_fix_contiguity(pmmg_hip_ctx *c, int ne, const int *tetv, const int *adja, const int *tet8, int *part,
                            int ncolor, int64_t *nmoved, int *nmerged, int *nstuck) {
  if (!enter(c)) return 0;
  TetView m;
  if (!contig_args(c, "fix_contiguity", ne, tetv, adja, tet8, part, ncolor, &m)) return 0;
  if (!nmoved || !nmerged || !nstuck) {
    set_err(c, "fix_contiguity: invalid arguments (a NULL counter)");
    return 0;
  }
  return pmmg_contig_fix(c->stream, m, part, ncolor, nmoved, nmerged, nstuck, &c->contig_cache, &c->snap_cache,
                         c->err, sizeof(c->err));
}

int64_t pmmg_hip_contig_passes(pmmg_hip_ctx *c) { return c ? c->contig_cache.passes : -1; }

// ---- group split (pmmg_split.hip)

int pmmg_hip_split_groups(pmmg_hip_ctx *c, int np, int ne, const int *tetv, const int *adja, const int *tet8,
                          const int *part, int ngrp, const int *node_pos, const int *face_old, int nnode0, int nface0,
                          pmmg_hip_split_count *count, int64_t pt_cap, int64_t face_cap, int64_t node_cap, int *old_tet,
                          int *new_tet, int *tetv_out, int *adja_out, int *tet8_out, int *old_pt, int *face_idx1,
                          int *face_idx2, int *node_idx1, int *node_idx2, int *nnode_end, int *nface_end) {
  if (!enter(c)) return 0;
  SplitArgs a{np, TetView{}, part, ngrp, node_pos, face_old, nnode0, nface0, count, pt_cap, face_cap, node_cap,
              old_tet, new_tet, tetv_out, adja_out, tet8_out, old_pt, face_idx1, face_idx2, node_idx1, node_idx2,
              nnode_end, nface_end};
  const TetArgs ta = tet_view(ne, tetv, adja, tet8, TET_NEED_TETV | TET_NEED_ADJA, &a.m);
  if (np < 0 || ne < 0 || ngrp < 1 || nnode0 < 0 || nface0 < 0 || !count || !nnode_end || !nface_end || pt_cap < 0 ||
      face_cap < 0 || node_cap < 0 || ta == TET_MISSING || (ne > 0 && (np < 1 || !part || !old_tet))) {
    set_err(c, "split_groups: invalid arguments (np=%d ne=%d ngrp=%d nnode0=%d nface0=%d)", np, ne, ngrp, nnode0,
            nface0);
    return 0;
  }
  if (ta == TET_TOOMANY) {
    set_err(c, "split_groups: %d tetra exceed the 4*k+i adjacency encoding (2^29)", ne);
    return 0;
  }
  if (ta == TET_MISALIGNED || !aligned<16>(tetv_out) || !aligned<16>(adja_out) || !aligned<16>(tet8_out)) {
    set_err(c, "split_groups: device tetra arrays (in and out) must be 16-byte aligned");
    return 0;
  }
  for (const void *p : {(const void *)part, (const void *)node_pos, (const void *)face_old, (const void *)old_tet,
                        (const void *)new_tet, (const void *)old_pt, (const void *)face_idx1, (const void *)face_idx2,
                        (const void *)node_idx1, (const void *)node_idx2})
    if (!aligned<4>(p)) {
      set_err(c, "split_groups: part, the positions and the lists must be 4-byte aligned");
      return 0;
    }
  return pmmg_split_groups(c->stream, a, &c->split_cache, c->err, sizeof(c->err));
}

// the two gathers (pmmg_gather.hip): rows of `size` elements of `elem` bytes; `unaligned` is the call's own text
static int gather_rows(pmmg_hip_ctx *c, const char *who, const char *unaligned, int64_t n, const int *src, int size,
                       int elem, const void *in, void *out) {
  if (!enter(c)) return 0;
  if (n < 0 || size < 1 || (n > 0 && (!src || !in || !out))) {
    set_err(c, "%s: invalid arguments (n=%lld size=%d)", who, (long long)n, size);
    return 0;
  }
  if (!aligned<4>(src) || ((uintptr_t)in | (uintptr_t)out) % (uintptr_t)elem) {
    set_err(c, "%s: %s", who, unaligned);
    return 0;
  }
  if (!pmmg_gather_rows(c->stream, n, src, (int64_t)size * elem, elem, in, out, c->err, sizeof(c->err))) return 0;
  HIPCK(c, hipStreamSynchronize(c->stream));
  return 1;
}

int pmmg_hip_gather_rows(pmmg_hip_ctx *c, int64_t n, const int *src, int size, const double *in, double *out) {
  return gather_rows(c, "gather_rows", "src must be 4-byte, in / out 8-byte aligned", n, src, size, 8, in, out);
}

int pmmg_hip_split_rounds(pmmg_hip_ctx *c) { return c ? c->split_cache.rounds : -1; }

// ---- group merge (pmmg_merge.hip)

int pmmg_hip_merge_groups(pmmg_hip_ctx *c, int ngrp, const pmmg_hip_split_count *count, const int *tetv, const int *tet8,
                          const int *node_idx1, const int *node_idx2, const int *face_idx1, const int *face_idx2,
                          int nnode, int nface, const int *color, int64_t pt_cap, int *new_pt, int *new_tet, int *src_pt,
                          int *src_tet, int *tetv_out, int *mark_out, int *node_val, int *face_val, int *np_out,
                          int *ne_out) {
  if (!enter(c)) return 0;
  if (ngrp < 1 || !count || nnode < 0 || nface < 0 || pt_cap < 0 || !np_out || !ne_out || (!color && mark_out)) {
    set_err(c, "merge_groups: invalid arguments (ngrp=%d nnode=%d nface=%d pt_cap=%lld, a NULL count or counter, or "
               "mark_out without color)", ngrp, nnode, nface, (long long)pt_cap);
    return 0;
  }
  if (nnode >= kTetMax || nface >= kTetMax) {
    set_err(c, "merge_groups: %d node or %d face positions reach 2^29", nnode, nface);
    return 0;
  }
  int64_t tot[4] = {0, 0, 0, 0};
  for (int g = 0; g < ngrp; g++) {
    tot[0] += count[g].ne > 0;
    tot[1] += count[g].np > 0;
    tot[2] += count[g].nface > 0;
    tot[3] += count[g].nnode > 0;
  }
  if ((tot[0] && ((!tetv && !tet8) || !src_tet)) || (tot[1] && !new_pt) || (tot[2] && (!face_idx1 || !face_idx2)) ||
      (tot[3] && (!node_idx1 || !node_idx2))) {
    set_err(c, "merge_groups: invalid arguments (an array with entries is NULL)");
    return 0;
  }
  const int *rows = tet8 ? tet8 : tetv;
  if (!aligned<16>(rows) || !aligned<16>(tetv_out)) {
    set_err(c, "merge_groups: device tetra arrays (in and out) must be 16-byte aligned");
    return 0;
  }
  for (const void *p : {(const void *)node_idx1, (const void *)node_idx2, (const void *)face_idx1,
                        (const void *)face_idx2, (const void *)new_pt, (const void *)new_tet, (const void *)src_pt,
                        (const void *)src_tet, (const void *)mark_out, (const void *)node_val, (const void *)face_val})
    if (!aligned<4>(p)) {
      set_err(c, "merge_groups: the lists, the maps and the values must be 4-byte aligned");
      return 0;
    }
  const MergeArgs a{ngrp, count, rows, tet8 ? 2 : 1, node_idx1, node_idx2, face_idx1, face_idx2, nnode, nface, color,
                    pt_cap, new_pt, new_tet, src_pt, src_tet, tetv_out, mark_out, node_val, face_val, np_out, ne_out};
  return pmmg_merge_groups(c->stream, a, &c->merge_cache, c->err, sizeof(c->err));
}

int pmmg_hip_gather_rows_i32(pmmg_hip_ctx *c, int64_t n, const int *src, int size, const int *in, int *out) {
  return gather_rows(c, "gather_rows_i32", "src, in and out must be 4-byte aligned", n, src, size, 4, in, out);
}

// ---- interface displacement (pmmg_moveifc.hip)

// the arguments the three calls share; fills *m
static int ifc_args(pmmg_hip_ctx *c, const char *who, int np, int ne, const int *tetv, const int *tet8, const int *mark,
                    int ncolor, const void *host, TetView *m) {
  const TetArgs ta = tet_view(ne, tetv, nullptr, tet8, TET_NEED_TETV, m);
  if (np < 0 || ne < 0 || ncolor < 1 || !host || ta == TET_MISSING || (ne > 0 && !mark)) {
    set_err(c, "%s: invalid arguments (np=%d ne=%d ncolor=%d)", who, np, ne, ncolor);
    return 0;
  }
  if (ta == TET_TOOMANY) {
    set_err(c, "%s: %d tetra exceed the 4*k+i corner encoding (2^29)", who, ne);
    return 0;
  }
  if ((ne > 0 && !aligned<16>(m->tetv)) || !aligned<4>(mark)) {
    set_err(c, "%s: device tetra arrays must be 16-byte, every other int array 4-byte aligned", who);
    return 0;
  }
  return 1;
}

int pmmg_hip_ifc_seed(pmmg_hip_ctx *c, int np, int ne, const int *tetv, const int *tet8, const int *mark, int ncolor,
                      const int *weight, int *ptcolor, unsigned char *ptfront) {
  if (!enter(c)) return 0;
  TetView m;
  if (!ifc_args(c, "ifc_seed", np, ne, tetv, tet8, mark, ncolor, weight, &m)) return 0;
  if (np > 0 && (!ptcolor || !ptfront || !aligned<4>(ptcolor))) {
    set_err(c, "ifc_seed: invalid arguments (ptcolor / ptfront NULL, or ptcolor not 4-byte aligned)");
    return 0;
  }
  return pmmg_ifc_seed(c->stream, np, m, mark, ncolor, weight, ptcolor, ptfront, &c->move_cache, c->err, sizeof(c->err));
}

int pmmg_hip_ifc_layers(pmmg_hip_ctx *c, int np, int ne, const int *tetv, const int *tet8, int *mark, int ncolor,
                        const int *weight, int *nelem, const int *nemin, int *ptcolor, unsigned char *ptfront, int nset,
                        const int *set_pt, const int *set_color, int nlayers, int *layers_done, int *blocked,
                        int *moved) {
  if (!enter(c)) return 0;
  TetView m;
  if (!ifc_args(c, "ifc_layers", np, ne, tetv, tet8, mark, ncolor, weight, &m)) return 0;
  if (!nelem || !nemin || !layers_done || !blocked || nlayers < 0 || (nlayers > 0 && !moved) || nset < 0 ||
      (nset > 0 && !set_pt) || (np > 0 && (!ptcolor || !ptfront))) {
    set_err(c, "ifc_layers: invalid arguments (nset=%d nlayers=%d, or a NULL array)", nset, nlayers);
    return 0;
  }
  if (!aligned<4>(ptcolor) || !aligned<4>(set_pt) || !aligned<4>(set_color)) {
    set_err(c, "ifc_layers: device tetra arrays must be 16-byte, every other int array 4-byte aligned");
    return 0;
  }
  return pmmg_ifc_layers(c->stream, np, m, mark, ncolor, weight, nelem, nemin, ptcolor, ptfront, nset, set_pt,
                         set_color, nlayers, layers_done, blocked, moved, &c->move_cache, c->err, sizeof(c->err));
}

int pmmg_hip_remap_colors(pmmg_hip_ctx *c, int ne, const int *tetv, const int *tet8, const int *mark, int ncolor,
                          const int *order, int *part, int *ngrp) {
  if (!enter(c)) return 0;
  TetView m;
  if (!ifc_args(c, "remap_colors", 0, ne, tetv, tet8, mark, ncolor, order, &m)) return 0;
  if (!ngrp || (ne > 0 && !part) || !aligned<4>(part)) {
    set_err(c, "remap_colors: invalid arguments (ngrp / part NULL, or part not 4-byte aligned)");
    return 0;
  }
  return pmmg_ifc_remap(c->stream, m, mark, ncolor, order, part, ngrp, &c->move_cache, c->err, sizeof(c->err));
}

int pmmg_hip_build_boundary(pmmg_hip_ctx *c, int np, int ne, const int *tet8, const int *tetv, const int *adja,
                            const int *tref, int cap, int *nt, int *triv, int *adjt) {
  if (!enter(c)) return 0;
  TetView m;
  const TetArgs ta = tet_view(ne, tetv, adja, tet8, TET_NEED_TETV | TET_NEED_ADJA | TET_ANY_NE, &m);
  if (np <= 0 || ne <= 0 || !nt || ta == TET_MISSING || cap < 0 || (cap > 0 && !triv)) {
    set_err(c, "build_boundary: invalid arguments (np=%d ne=%d cap=%d)", np, ne, cap);
    return 0;
  }
  if (ta == TET_MISALIGNED) {
    set_err(c, "build_boundary: device tetra arrays must be 16-byte aligned");
    return 0;
  }
  return pmmg_snap_boundary(c->stream, np, m, tref, cap, nt, triv, adjt, &c->snap_cache, c->err, sizeof(c->err));
}

void *pmmg_hip_malloc(pmmg_hip_ctx *c, int64_t bytes) {
  if (!c || bytes < 0) return nullptr;
  if (hipSetDevice(c->device) != hipSuccess) return nullptr;
  void *p = nullptr;
  if (hipMalloc(&p, bytes > 0 ? (size_t)bytes : 16) != hipSuccess) {
    set_err(c, "hipMalloc(%lld) failed", (long long)bytes);
    return nullptr;
  }
  return p;
}

int pmmg_hip_free(pmmg_hip_ctx *c, void *p) {
  if (!enter(c)) return 0;
  HIPCK(c, hipFree(p));
  return 1;
}

int pmmg_hip_memcpy_h2d(pmmg_hip_ctx *c, void *dst, const void *src, int64_t bytes) {
  if (bytes < 0 || !enter(c)) return 0;
  if (!h2d(c, dst, src, (size_t)bytes, c->stream)) return 0;
  HIPCK(c, hipStreamSynchronize(c->stream));
  return 1;
}

// ---- the split of a group over the node's GPUs (pmmg_comm.hpp)

int pmmg_hip_comm_unique_id(void *id) {
  if (!id) return 0;
  Rccl &R = rccl();
  if (!R.ok) {
    fprintf(stderr, "[parmmg_hip] comm_unique_id: %s\n", R.why);
    return 0;
  }
  ncclUniqueId u;
  const ncclResult_t e = R.getUniqueId(&u);
  if (e != ncclSuccess) {
    fprintf(stderr, "[parmmg_hip] ncclGetUniqueId: %s\n", R.errorString(e));
    return 0;
  }
  memcpy(id, &u, sizeof(u));
  return 1;
}

int pmmg_hip_comm_init(pmmg_hip_ctx *c, int nranks, int rank, const void *id) {
  if (!enter(c)) return 0;
  if (nranks < 1 || rank < 0 || rank >= nranks || !id) {
    set_err(c, "comm_init: invalid arguments (nranks=%d rank=%d)", nranks, rank);
    return 0;
  }
  Rccl &R = rccl();
  if (!R.ok) {
    set_err(c, "comm_init: %s", R.why);
    return 0;
  }
  comm_release(c);
  ncclUniqueId u;
  memcpy(&u, id, sizeof(u));
  ncclComm_t comm = nullptr;
  const ncclResult_t e = R.commInitRank(&comm, nranks, u, rank);
  if (e != ncclSuccess) {
    set_err(c, "ncclCommInitRank(%d of %d): %s", rank, nranks, R.errorString(e));
    return 0;
  }
  c->comm = comm;
  c->comm_owned = true;
  c->comm_rank = rank;
  c->comm_size = nranks;
  // the all-gather's agreement buffer, allocated here so that pmmg_hip_allgather_points allocates nothing
  // before every rank has agreed (ag_agree)
  return ensure(c, c->ag_chk, sizeof(long long) * kAgView * (nranks + 1));
}

int pmmg_hip_comm_attach(pmmg_hip_ctx *c, void *comm, int nranks, int rank) {
  if (!c) return 0;
  if (nranks < 1 || rank < 0 || rank >= nranks || !comm) {
    set_err(c, "comm_attach: invalid arguments (nranks=%d rank=%d)", nranks, rank);
    return 0;
  }
  if (!rccl().ok) {
    set_err(c, "comm_attach: %s", rccl().why);
    return 0;
  }
  comm_release(c);
  c->comm = (ncclComm_t)comm;
  c->comm_owned = false;
  c->comm_rank = rank;
  c->comm_size = nranks;
  return ensure(c, c->ag_chk, sizeof(long long) * kAgView * (nranks + 1)); // (see pmmg_hip_comm_init)
}

int pmmg_hip_allgather_points(pmmg_hip_ctx *c, const int64_t *counts, int nslot, const int *slot_size,
                              const double *const *rows, double *const *rows_all, const int *elem, int *elem_all,
                              const int8_t *hit, int8_t *hit_all) {
  return enter(c) && ag_points(c, counts, nslot, slot_size, rows, rows_all, elem, elem_all, hit, hit_all);
}

int pmmg_hip_memcpy_d2h(pmmg_hip_ctx *c, void *dst, const void *src, int64_t bytes) {
  if (bytes < 0 || !enter(c)) return 0;
  if ((size_t)bytes < kStageMin) {
    HIPCK(c, hipMemcpyAsync(dst, src, (size_t)bytes, hipMemcpyDeviceToHost, c->stream));
    HIPCK(c, hipStreamSynchronize(c->stream));
    return 1;
  }
  return d2h_rows(c, dst, src, (size_t)bytes, 1, AllRows{});
}

} // extern "C"
