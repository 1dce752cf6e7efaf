// pmmg_call.hpp — one pmmg_hip_locate_interp on device pointers (included by pmmg_hip.hip only): the slot layouts
// the volume kernel is compiled for, the call's state with the record of its events, its stages in the order they
// run, run_device, and the statistics read back from the call's events.
#pragma once

#include <hip/hip_ext.h> // hipExtLaunchKernelGGL: events recorded by the kernel dispatch itself

#include "pmmg_xfer.hpp" // k_fill64, kRefillCells
#include "pmmg_sort.hpp"
#include "pmmg_vol.hpp"
#include "pmmg_bdy.hpp"
#include "pmmg_fallback.hpp"

namespace {

// ---------------------------------------------------------------- slot layouts

typedef void (*VolFn)(Bg, const Frame *, const unsigned long long *, int, const double *, const uint8_t *,
                      const int *, int, DevStats *, Slots, int *, int8_t *, int, const int *, int, ContArgs, MapArgs);

struct LayoutEntry {
  int c[6];
  VolFn fn;         // one array per solution (the reference's layout)
  VolFn fn_packed;  // packed per-vertex records, one pass (null: layout not packable)
  VolFn fn_packed2; // the same in two passes over the record halves (null: not splittable)
  VolFn map_fn, map_fn_packed, map_fn_packed2; // the same three for a call with a point map (k_vol's MAP)
};

template <int NP, int A, int B, int C, int D, int E, int F, int MAP = 0>
constexpr VolFn packed_fn() {
  using L = PackedLayout<A, B, C, D, E, F>;
  if constexpr (L::valid() && L::passes_ok(NP)) return k_vol<NP, A, B, C, D, E, F, MAP>;
  else return nullptr;
}
#define PMMG_LAYOUT(a, b, c, d, e, f)                                                                    \
  {{a, b, c, d, e, f}, k_vol<0, a, b, c, d, e, f>, packed_fn<1, a, b, c, d, e, f>(),                    \
   packed_fn<2, a, b, c, d, e, f>(), k_vol<0, a, b, c, d, e, f, 1>, packed_fn<1, a, b, c, d, e, f, 1>(), \
   packed_fn<2, a, b, c, d, e, f, 1>()}
// common slot layouts (metric first): aniso metric + scalar/vector/tensor
// (BASELINE cfg3/cfg4, libexamples cube-solphys.sol), iso metric + scalars
// (cfg2, cfg5), metric only; anything else runs the runtime-layout variant
const LayoutEntry kLayouts[] = {
    PMMG_LAYOUT(6, 1, 3, 6, 0, 0), PMMG_LAYOUT(6, 1, 3, 6, 1, 0), PMMG_LAYOUT(1, 1, 0, 0, 0, 0),
    PMMG_LAYOUT(1, 1, 1, 1, 1, 1), PMMG_LAYOUT(1, 1, 1, 0, 0, 0), PMMG_LAYOUT(6, 0, 0, 0, 0, 0),
    PMMG_LAYOUT(1, 0, 0, 0, 0, 0), PMMG_LAYOUT(6, 1, 0, 0, 0, 0), PMMG_LAYOUT(1, 1, 3, 6, 0, 0),
    PMMG_LAYOUT(0, 0, 0, 0, 0, 0), // locate only (no metric, no field)
};
#undef PMMG_LAYOUT

// passes: packed records' gather passes (1 or 2; the other is taken when the
// layout allows only it; 0 = by the record's size: two above 8 doubles, where
// one pass holds the whole record in registers — cfg4's 16 doubles: 168
// VGPRs, 3 waves per SIMD, 4.42 ms per step against 4.18 in two passes, r05d)
VolFn pick_layout(const Slots &S, int passes = 0, bool map = false) {
  for (const LayoutEntry &e : kLayouts) {
    int n = 0;
    while (n < 6 && e.c[n] > 0) n++;
    if (n != S.n) continue;
    bool ok = true;
    for (int j = 0; j < n; j++) ok = ok && (S.s[j].code == e.c[j]);
    if (!ok) continue;
    if (!S.rec) return map ? e.map_fn : e.fn;
    if (passes == 0) {
      int k = 0;
      for (int j = 0; j < n; j++) k += e.c[j];
      passes = k > 8 ? 2 : 1;
    }
    const VolFn p1 = map ? e.map_fn_packed : e.fn_packed, p2 = map ? e.map_fn_packed2 : e.fn_packed2;
    const VolFn a = passes == 2 ? p2 : p1, b = passes == 2 ? p1 : p2;
    return a ? a : b;
  }
  if (S.rec) return nullptr;
  return map ? k_vol<0, -1, 0, 0, 0, 0, 0, 1> : k_vol<0, -1, 0, 0, 0, 0, 0>;
}

// the slot layouts the packed-record interpolation is compiled for
bool packed_supported(int met_size, int nfield, const int *fsize) {
  Slots S{};
  S.rec = reinterpret_cast<const double *>(16);
  if (met_size) S.s[S.n++].code = met_size;
  for (int j = 0; j < nfield && S.n < kMaxSlot; j++) S.s[S.n++].code = fsize[j];
  return pick_layout(S) != nullptr;
}

} // namespace

// groups with fewer new points take the input order without the coherence
// test: their background stays in the caches, and the binning costs more
// than a numbering's locality (r04g, shuffled numberings: cfg2's 205k points
// 0.19 ms per call in input order, 0.31 Morton-binned; cfg3's 4.1M points
// 2.74 vs 1.89 ms)
constexpr int kSmallGroup = 1 << 20;

// The background's start tables (pmmg_prep.hpp: point map), built on the
// main stream when the background has none yet: start_tet[np], start_tri[np].
static int start_tables(pmmg_hip_ctx *c) {
  if (c->start_valid) return 1;
  const Bg &bg = c->bg;
  const size_t n = 2 * (size_t)bg.np;
  if (!ensure(c, c->start_tab, sizeof(int) * n)) return 0;
  unsigned *tab = c->start_tab.as<unsigned>();
  HIPCK(c, hipMemsetAsync(tab, 0xFF, sizeof(int) * n, c->stream));
  hipLaunchKernelGGL(k_start_tet, dim3(blocks_for(bg.ne, 16384)), dim3(kBlock), 0, c->stream, bg, tab);
  if (bg.nt > 0)
    hipLaunchKernelGGL(k_start_tri, dim3(blocks_for(bg.nt, 4096)), dim3(kBlock), 0, c->stream, bg, tab + bg.np);
  hipLaunchKernelGGL(k_start_fin, dim3(blocks_for((long long)n, 4096)), dim3(kBlock), 0, c->stream, tab, (long long)n);
  HIPCK(c, hipGetLastError());
  c->start_valid = true;
  return 1;
}

// ---------------------------------------------------------------- one call on device pointers
//
// run_device enqueues one call's kernels on the context's streams, stage by
// stage (the functions below, in the order they run); every fallback kernel
// reads its list's count on the device.  Only a large call in auto order mode
// reads something back: the coherence test's decision, once (run_device).

// Measured settings, runtime arguments of the kernels that take them
constexpr int kSeedLanes = 4;    // sampled tetra per seed run of 4 records (1..4)
constexpr int kBboxStride = 64;  // the frame's bbox samples np / 64 vertices (r03o: 64 instead of 16 and
constexpr int kHistStride = 256; // 256 instead of 64 for the axis histograms: preparation -0.15 ms at cfg4, same walks)
constexpr int kBdyBpx = 512;     // k_bdy blocks per XCD at most, in blocks of kBlock threads
constexpr int kXcdRun = 64;      // k_vol's blocks dealt to the XCDs in runs of 64 (4096 queries) instead of contiguous
                                 // eighths: r04c at cfg4, volume kernel 3.80 -> 3.50 ms, Mmg-like numbering 5.83 -> 4.14 ms

// One call's arguments and what its stages share
struct Call {
  pmmg_hip_ctx *c;
  int np_new;
  const double *xyz_new;
  const uint8_t *pclass;
  int *elem_out;
  int8_t *hit_out;
  Bg bg;                 // the context's background with the call's fixed-point copy (xq)
  hipStream_t s, sb, sc; // main stream, surface stream, the Morton binning's stream (sb when it has none of its own)
  Slots S;
  VolFn vol_fn;
  MapArgs ma; // a call with a point map (else nulls)
  int *need;  // its counts of queries the map gives no start {volume, surface}, which gate the seed grids (else null)
  int force;  // the query order: 1 Morton, 0 input; -1 while a large auto-order call's decision is on its way
  int g, gs;  // cells per axis of the volume / surface seed grid
  long long ng, nsg, ncls; // their cells; blocks of the surface list's compaction
  Frame *fr;
  DevStats *st;
  unsigned long long *grid, *sgrid;
  int *order_v, *order_b;
  const int *flag; // the order decision on the device {sorted, bits per axis}

  // The events this call has recorded, bit by bit.  The events belong to the context and outlive the call: a wait
  // for one that this call did not record would be satisfied by an earlier call's record and do nothing, so every
  // event operation of a call goes through the members below (the host's one wait, for EV_FRAME, asks recorded()).
  unsigned evs;
  bool has(int ev) const { return (evs >> ev) & 1u; }
  // ev as the start or stop event of a kernel's dispatch: named in the launch statement itself
  hipEvent_t mark(int ev) {
    evs |= 1u << ev;
    return c->ev[ev];
  }
  int rec(int ev, hipStream_t st) { // a marker
    HIPCK(c, hipEventRecord(mark(ev), st));
    return 1;
  }
  int recorded(int ev) const { // 1, or 0 with the call failed
    if (!has(ev)) set_err(c, "locate_interp: internal: wait for event %d, which this call has not recorded", ev);
    return has(ev);
  }
  int wait(hipStream_t st, int ev) {
    if (!recorded(ev)) return 0;
    HIPCK(c, hipStreamWaitEvent(st, c->ev[ev], 0));
    return 1;
  }
};

// The exhaustive searches of one class (NV = 4: the volume queries' on the main stream after the exact continuation,
// 3: the surface queries' on the surface stream after k_bdy): the list's query grid, then the accepting and the
// closest search, the last of which records `stop`.  The lists and their counts live on the device, every kernel
// reads its; the grid is sized by the background (fb_blocks).
template <int NV>
static void launch_fallbacks(Call &k, hipStream_t s, hipEvent_t stop) {
  using E = FbElem<NV>;
  const Bg &bg = k.c->bg;
  const FbBufs &f = k.c->fb[E::cls];
  const int *fb = f.list.as<const int>();
  const int blocks = fb_blocks<NV>(E::count(bg));
  hipLaunchKernelGGL(k_fb_grid, dim3(1), dim3(kBlock), 0, s, k.xyz_new, fb, k.st, E::cls, f.grid());
  hipLaunchKernelGGL(k_exhaust_accept<NV>, dim3(blocks), dim3(kBlock), 0, s, bg, k.xyz_new, fb, k.st,
                     f.best.as<int>(), f.nac.as<int>(), f.g_cells.as<const int>(), f.g_items.as<const int>(), k.S,
                     k.elem_out, k.hit_out);
  hipExtLaunchKernelGGL(k_exhaust_closest<NV>, dim3(blocks), dim3(kBlock), 0, s, nullptr, stop, 0, bg, k.xyz_new, fb,
                        k.st, f.nac.as<const int>(), f.part.as<FbPart>(), f.cres.as<int>(), k.S, k.elem_out,
                        k.hit_out);
}

// ---- slots and layout: the arguments checked, the solutions' slots, the volume kernel for their layout, the
// point map's start tables
static int call_slots(Call &k, double *met_out, double *const *fields_out, double *rec_out, const int *map_src) {
  pmmg_hip_ctx *c = k.c;
  Slots &S = k.S;
  S.n = 0;
  S.has_met = c->met_size ? 1 : 0;
  if (rec_out && !c->rec) {
    set_err(c, "locate_interp_rec: output records need packed input records (pmmg_hip_set_solutions_packed)");
    return 0;
  }
  if (c->met_size) {
    if (!met_out && !rec_out) {
      set_err(c, "locate_interp: met_out is NULL");
      return 0;
    }
    S.s[S.n++] = Slot{c->met, met_out, c->met_size, c->met_size, c->met_size};
  }
  for (int j = 0; j < c->nfield; j++) {
    if (!rec_out && (!fields_out || !fields_out[j])) {
      set_err(c, "locate_interp: fields_out[%d] is NULL", j);
      return 0;
    }
    S.s[S.n++] = Slot{c->fin[j], rec_out ? nullptr : fields_out[j], c->fsize[j], c->fsize[j], c->fsize[j]};
  }
  if (c->rec) { // packed records: every slot reads its columns of the record
    S.rec = c->rec;
    int off = 0;
    for (int j = 0; j < S.n; j++) {
      S.s[j].in = c->rec + off;
      S.s[j].istride = c->rstride;
      if (rec_out) { // and writes its columns of the new point's output record
        S.s[j].out = rec_out + off;
        S.s[j].ostride = c->rstride;
      }
      off += S.s[j].code;
    }
    S.rec_out = rec_out;
  }
  k.vol_fn = pick_layout(S, c->pack_passes, map_src != nullptr);
  if (!k.vol_fn) {
    set_err(c, "locate_interp: no packed-record kernel for this slot layout");
    return 0;
  }
  // a call with a point map: the background's start tables (built now if it has none), and the counts of
  // queries the map gives no start, which gate the seed grids on the device
  k.ma = MapArgs{nullptr, nullptr, nullptr};
  k.need = nullptr;
  if (map_src) {
    if (!start_tables(c) || !ensure(c, c->map_need, 2 * sizeof(int))) return 0;
    k.need = c->map_need.as<int>();
    k.ma = MapArgs{map_src, c->start_tab.as<const int>(), c->start_tab.as<const int>() + k.bg.np};
  }
  return 1;
}

// one family's buffers for a call of nq queries (nparts: the closest search's range minima)
static int fb_scratch(pmmg_hip_ctx *c, FbBufs &f, size_t nq, size_t nparts) {
  return ensure(c, f.list, 4 * nq) && ensure(c, f.best, 4 * nq) && ensure(c, f.nac, 4 * nq) &&
         ensure(c, f.cres, 4 * nq) && ensure(c, f.part, sizeof(FbPart) * nparts) &&
         ensure(c, f.g_cells, 4 * (size_t)(kFbCells + 1)) && ensure(c, f.g_cur, 4 * (size_t)kFbCells) &&
         ensure(c, f.g_items, 4 * nq);
}

// ---- scratch: the grids' sizes, the work buffers, the query order known at entry
static int call_scratch(Call &k) {
  pmmg_hip_ctx *c = k.c;
  Bg &bg = k.bg;
  k.g = grid_dim(bg.ne, c->tpc, 1024);
  k.gs = bg.nt <= 0 ? 1 : (c->srf_g > 0 ? c->srf_g : grid_dim((long long)bg.nt * c->srf_mult, 2, 1024));
  const size_t nq = (size_t)k.np_new;
  k.ng = (long long)k.g * k.g * k.g;
  k.nsg = bg.nt > 0 ? (long long)k.gs * k.gs * k.gs : 0;
  k.ncls = (long long)(nq / kScanChunk + 1);
  if (!ensure(c, c->frame, sizeof(Frame)) || !ensure(c, c->stats, sizeof(DevStats) + kStatParts * sizeof(StatPart)) ||
      !ensure(c, c->grid, 8 * (size_t)k.ng) || !ensure(c, c->sgrid, 8 * (size_t)k.nsg) ||
      !ensure(c, c->order_v, 4 * nq) || !ensure(c, c->order_b, 4 * nq) || !ensure(c, c->bkeys, 4 * nq) ||
      !ensure(c, c->bkeys2, 4 * nq) || !ensure(c, c->bvals, 4 * nq) || !ensure(c, c->cls_cnt, 4 * (size_t)k.ncls) ||
      !fb_scratch(c, c->fb[0], nq, kFbPartCap<4>) || !fb_scratch(c, c->fb[1], nq, kFbPartCap<3>))
    return 0;
  if (!ensure(c, c->xq, sizeof(int) * kXqStride * (size_t)bg.np) || !ensure(c, c->oflag, 2 * sizeof(int)) ||
      !ensure(c, c->cohd, sizeof(double) * kCohSamples) ||
      !ensure(c, c->axh, sizeof(int) * 3 * kMapBins * (size_t)kHistBlocks))
    return 0;
  bg.xq = c->xq.as<const int>();
  k.fr = c->frame.as<Frame>();
  k.st = c->stats.as<DevStats>();
  k.grid = c->grid.as<unsigned long long>();
  k.sgrid = c->sgrid.as<unsigned long long>();
  k.order_v = c->order_v.as<int>();
  k.order_b = c->order_b.as<int>();
  k.flag = c->oflag.as<const int>();
  // Forced orders enqueue only theirs; a small group (below kSmallGroup queries: its background and solutions
  // stay in the Infinity Cache, where a numbering's locality matters little) takes the input order untested.
  k.force = (c->options & PMMG_HIP_OPT_SORT) ? 1 : (c->options & PMMG_HIP_OPT_NOSORT) ? 0 : -1;
  if (k.force < 0 && k.np_new < kSmallGroup) k.force = 0;
  // r06: a large auto-order call reads the decision back once k_bbox is done (the host waits while the device
  // runs the fixed-point copy and the seed grid, ~0.4 ms at cfg4) and enqueues only the chosen order's
  // kernels.  With both orders enqueued and gated on the device, the input order's volume kernel waited for
  // the ~19 gated binning launches (each dispatched only when the preparation kernels left a slot free: they
  // ended 20-55 us after the seed grid, profiles/r06i, r06k), or, below 2^23 queries, the other order's
  // volume launch returned at once in 40-64k one-wave blocks (~35-55 us of dispatch on the main stream).
  if (k.force < 0 && !c->flag_host) {
    void *p = nullptr;
    HIPCK(c, hipHostMalloc(&p, 64, hipHostMallocCoherent | hipHostMallocMapped));
    c->flag_host = (int *)p;
    void *d = nullptr;
    HIPCK(c, hipHostGetDevicePointer(&d, p, 0));
    c->flag_host_dev = (int *)d;
  }
  if (k.force < 0) c->flag_host[0] = -1;
  return 1;
}

// ---- frame and seeds (main stream): reset, the map's counts, the frame with the coherence test, the fixed-point
// copy and the axis maps, the volume seed grid; the other streams are told what to wait for in between.
// The call's events ride on its kernels' dispatches where a kernel is at hand (hipExtLaunchKernelGGL start /
// stop events): a separate marker between two kernels of a stream cost the device ~4 us, an event on the
// dispatch ~1.7 (tools/calib/ext_event.hip, profiles/r06zj)
static int launch_frame_seeds(Call &k) {
  pmmg_hip_ctx *c = k.c;
  const Bg &bg = k.bg;
  const int force = k.force;
  hipStream_t s = k.s;
  // seed grids: cleared here unless the previous call left them clean (a
  // large grid is refilled at the end of the call that used it, beside the
  // other stream's tail: r05, cfg4 k_reset 32 us -> the stats only)
  const long long ng_clr = (c->grid.p == c->grid_clean_p && k.ng <= c->grid_clean_n) ? 0 : k.ng;
  const long long nsg_clr = (c->sgrid.p == c->sgrid_clean_p && k.nsg <= c->sgrid_clean_n) ? 0 : k.nsg;
  c->grid_clean_n = c->sgrid_clean_n = 0; // dirty until this call's refill is enqueued
  // the input order's surface list needs only the zeroed counters (and the coherence flag), not the frame
  // (r06: EV_RESET is waited for only in a forced order, EV_VOL0 only when a kernel separates it from EV_PREP)
  hipExtLaunchKernelGGL(k_reset, dim3(blocks_for(ng_clr > nsg_clr ? ng_clr : nsg_clr, 2048)), dim3(kBlock), 0, s,
                        k.mark(EV_START), force >= 0 ? k.mark(EV_RESET) : nullptr, 0, k.fr, k.st, k.grid, ng_clr,
                        k.sgrid, nsg_clr, c->oflag.as<int>(), force, c->bin_bits);
  if (k.need) {
    HIPCK(c, hipMemsetAsync(k.need, 0, 2 * sizeof(int), s));
    hipLaunchKernelGGL(k_map_count, dim3(blocks_for(k.np_new, 2048)), dim3(kBlock), 0, s, k.pclass,
                       (long long)k.np_new, k.ma, bg.np, bg.ne, bg.nt, k.need);
  }
  // bbox (its last block finalises the frame), the seed grid's axis maps
  // (auto order: the queries' coherence test rides along, its flag read by the order and volume kernels)
  // the second stream needs the frame only (lo, inv_bin, inv_srf), not the
  // axis maps (r04: EV_FRAME moved here from after k_axis_map)
  hipExtLaunchKernelGGL(k_bbox, dim3(std::max(force < 0 ? kCohBlocks : 1, blocks_for(bg.np / kBboxStride + 1, 256))),
                        dim3(kBlock), 0, s, nullptr, k.mark(EV_FRAME), 0, (const double *)bg.xyz, bg.np, k.fr,
                        kBboxStride, k.g, k.gs, 1 << kBinBitsAxis, k.xyz_new, k.np_new,
                        force < 0 ? c->oflag.as<int>() : nullptr, c->cohd.as<double>(),
                        force < 0 ? c->flag_host_dev : nullptr);
  // fixed-point vertex copy + the axis histograms (first kHistBlocks blocks), then the axis maps
  hipLaunchKernelGGL(k_quantize, dim3(std::max(kHistBlocks, blocks_for(3LL * bg.np, 8192))), dim3(kBlock), 0, s,
                     bg.xyz, (long long)bg.np, (const Frame *)k.fr, c->xq.as<int>(), kHistStride, c->axh.as<int>());
  hipLaunchKernelGGL(k_axis_map, dim3(3), dim3(kBlock), 0, s, c->axh.as<const int>(), k.fr, k.g);
  HIPCK(c, hipGetLastError());

  // the query order's stream (second stream, concurrent with the seed grid), after
  // the frame.  (r04: the axis maps moved here beside the fixed-point copy
  // cost 10 groups 0.11 -> 0.25 ms per group and the 8-way rank +0.02 ms for
  // -0.0 at cfg4, `profiles/r04s`: not kept)
  if (!k.wait(k.sb, force < 0 ? EV_FRAME : EV_RESET)) return 0; // (the order flag)
  // (EV_SB0: the start of the surface list's first kernel when there is one, launch_cls)
  if ((force == 1 || bg.nt <= 0) && !k.rec(EV_SB0, k.sb)) return 0;
  // the Morton binning on a third stream (r05, `profiles/r05m`: on the second stream its ~19 launches held the
  // 8-way rank's volume kernel 86 us behind the seed grid)
  k.sc = k.sb;
  if (force != 0) {
    if (!c->stream3 && hipStreamCreateWithFlags(&c->stream3, hipStreamNonBlocking) != hipSuccess)
      c->stream3 = nullptr;
    if (c->stream3) k.sc = c->stream3;
    if (!k.wait(k.sc, EV_FRAME)) return 0; // (the frame and the order flag)
  }
  HIPCK(c, hipGetLastError());

  // volume seeds
  const long long nsamp = k.ng < bg.ne ? k.ng : bg.ne;
  // kSeedBatch samples per thread in flight together (r05m: one per thread, the 8-way rank's 1.65M samples
  // took 107 us — the grid's latency in rounds of waves — where cfg4's 12.6M take 262 us)
  hipExtLaunchKernelGGL(k_seed_vol, dim3((blocks_for((nsamp + kSeedBatch - 1) / kSeedBatch, 8192) + 7) & ~7),
                        dim3(kBlock), 0, s, nullptr, k.mark(EV_PREP), 0, bg, k.fr, k.grid, k.g, nsamp, kSeedLanes,
                        (const int *)k.need);
  HIPCK(c, hipGetLastError());
  return 1;
}

// ---- order lists.  Input order: the surface points in input order (stable compaction: per-block counts, their
// scan, the scatter; rocPRIM's select took 0.2 ms longer here, r03o), second stream.  Its kernels are gated on
// the device flag: a large auto-order call launches them before its decision arrives.
// (EV_SB0 on its first kernel, EV_ORDER on its last)
static void launch_cls(Call &k) {
  if (k.force == 1 || k.bg.nt <= 0) return;
  int *bc = k.c->cls_cnt.as<int>();
  hipExtLaunchKernelGGL(k_cls_count, dim3((unsigned)k.ncls), dim3(kBlock), 0, k.sb, k.mark(EV_SB0), nullptr, 0,
                        k.pclass, (long long)k.np_new, (int)PMMG_PT_BDY, bc, k.flag, 0);
  hipLaunchKernelGGL(k_scan_top, dim3(1), dim3(kBlock), 0, k.sb, bc, (int)k.ncls, &k.st->nbdy, k.flag, 0);
  hipExtLaunchKernelGGL(k_cls_scatter, dim3((unsigned)k.ncls), dim3(kBlock), 0, k.sb, nullptr, k.mark(EV_ORDER), 0,
                        k.pclass, (long long)k.np_new, (int)PMMG_PT_BDY, (const int *)bc, k.order_b, k.flag, 0);
}

// Morton order: stable LSD radix sort of the keys (<= 3 * 7 + 2 bits) in 3 passes of 8 bits
// (pmmg_sort.hpp); the key kernel writes the first pass's digit table
static int launch_morton(Call &k) {
  pmmg_hip_ctx *c = k.c;
  const int np_new = k.np_new;
  if (k.force == 0 || np_new <= 0) return 1;
  hipStream_t sc = k.sc;
  const size_t nq = (size_t)np_new;
  const int ntile = (int)((np_new + kRsTile - 1) / kRsTile);
  const long long nh = 256LL * ntile;
  const int nch = (int)((nh + kScanChunk - 1) / kScanChunk);
  if (!ensure(c, c->bvals2, 4 * nq) || !ensure(c, c->rs_hist, 4 * (size_t)nh) || !ensure(c, c->rs_csum, 4 * (size_t)nch))
    return 0;
  unsigned *k0 = c->bkeys.as<unsigned>(), *k1 = c->bkeys2.as<unsigned>();
  int *v0 = c->bvals.as<int>(), *v1 = c->bvals2.as<int>(), *hist = c->rs_hist.as<int>(), *csum = c->rs_csum.as<int>();
  const int tgrid = std::min(ntile, kRsGrid);
  hipLaunchKernelGGL(k_bin_keys, dim3(tgrid), dim3(kBlock), 0, sc, k.xyz_new, k.pclass, np_new, (const Frame *)k.fr,
                     k.flag, k0, v0, k.st, kRsTile, ntile, hist);
  for (int pass = 0; pass < 3; pass++) {
    const unsigned *kin = pass == 1 ? k1 : k0;
    const int *vin = pass == 1 ? v1 : v0;
    unsigned *kout = pass == 1 ? k0 : k1;
    int *vout = pass == 1 ? v0 : (pass == 0 ? v1 : k.order_v);
    if (pass > 0)
      hipLaunchKernelGGL(k_rs_hist, dim3(tgrid), dim3(kBlock), 0, sc, kin, np_new, 8 * pass, ntile, hist, k.flag, 1);
    hipLaunchKernelGGL(k_rs_scan_local, dim3(nch), dim3(kBlock), 0, sc, hist, (int)nh, csum, k.flag, 1);
    hipLaunchKernelGGL(k_scan_top, dim3(1), dim3(kBlock), 0, sc, csum, nch, (int *)nullptr, k.flag, 1);
    hipLaunchKernelGGL(k_rs_scan_add, dim3(nch), dim3(kBlock), 0, sc, hist, (int)nh, (const int *)csum, k.flag, 1);
    hipLaunchKernelGGL(k_rs_scatter, dim3(tgrid), dim3(kBlock), 0, sc, kin, vin, np_new, 8 * pass, ntile,
                       (const int *)hist, kout, vout, k.flag, 1);
  }
  hipLaunchKernelGGL(k_bin_split, dim3(blocks_for(np_new, 4096)), dim3(kBlock), 0, sc, (const int *)k.order_v,
                     k.order_b, (const DevStats *)k.st, k.flag);
  return 1;
}

// ---- surface branch (second stream): seeds, k_bdy, its fallbacks, the surface grid's refill
// (r05ae: the surface seeds moved before the wait for the volume seed grid, beside it: preparation
// +0.03 ms at cfg4, +0.17 for the Mmg-like numbering, the 8-way rank +0.04 — not kept)
static int srf_head(Call &k) {
  const Bg &bg = k.bg;
  // a large call's surface branch waits for the volume seed grid (r04zo, cfg4: the seed grid ran at 455 instead
  // of 261 us beside k_bdy; step 4.24 -> 4.13 ms, Mmg-like 5.01 -> 4.93, shuffled =)
  if (k.np_new >= kSmallGroup && !k.wait(k.sb, EV_PREP)) return 0;
  if (bg.nt <= 0 && !k.rec(EV_BDY0, k.sb)) return 0; // (else the start of the surface seeds)
  if (bg.nt > 0) {
    if (k.force == 0 && !k.wait(k.sb, EV_FRAME)) return 0; // (the surface seeds need the frame)
    hipExtLaunchKernelGGL(k_seed_srf, dim3(blocks_for(bg.nt, 4096)), dim3(kBlock), 0, k.sb, k.mark(EV_BDY0), nullptr,
                          0, bg, (const Frame *)k.fr, k.sgrid, k.gs,
                          k.need ? (const int *)k.need + 1 : (const int *)nullptr);
  }
  return 1;
}

// one round of the grid for up to 1M surface points (static split: a
// second, nearly empty round doubled the surface branch alone)
static void launch_bdy(Call &k) {
  pmmg_hip_ctx *c = k.c;
  const auto bdy_fn = k.ma.src ? k_bdy<1> : k_bdy<0>;
  hipLaunchKernelGGL(bdy_fn, dim3(8 * blocks_for((k.np_new + 7) / 8, kBdyBpx)), dim3(kBlock), 0,
                     k.sb, k.bg, (const Frame *)k.fr, (const unsigned long long *)k.sgrid, k.gs, k.xyz_new,
                     (const int *)k.order_b, k.S, k.elem_out, k.hit_out, c->fb[1].list.as<int>(), k.st, c->maxstep,
                     c->fb[1].init(), k.ma);
}

// (EV_BDY1 on the branch's last launch, when it has one)
static int srf_tail(Call &k) {
  pmmg_hip_ctx *c = k.c;
  const bool fill = k.nsg >= kRefillCells;
  if (k.bg.nt > 0) {
    launch_fallbacks<3>(k, k.sb, fill ? nullptr : k.mark(EV_BDY1));
    HIPCK(c, hipGetLastError());
    if (fill) { // the surface grid refilled for the next call (see k_reset)
      hipExtLaunchKernelGGL(k_fill64, dim3(blocks_for((k.nsg + 1) / 2, 2048)), dim3(kBlock), 0, k.sb, nullptr,
                            k.mark(EV_BDY1), 0, k.sgrid, k.nsg, ~0ULL);
      c->sgrid_clean_p = c->sgrid.p;
      c->sgrid_clean_n = k.nsg;
    }
  }
  if (!k.has(EV_BDY1) && !k.rec(EV_BDY1, k.sb)) return 0;
  return 1;
}

// ---- volume stage (main stream): walk + exact test and continuation + interpolation in one kernel, whose
// dispatch records EV_WALK.  It reads the order branch's lists only in Morton order; in input order its queries
// are the input's volume points and there is nothing to wait for (r05: the cross-stream wait was ~20 us of a
// small group's main chain): launched right after the seed grid, the stage opens at EV_PREP.  In Morton order it
// waits for the lists (EV_ORDER2, on the surface stream when the binning has none of its own) and opens at EV_VOL0
static int launch_vol(Call &k) {
  pmmg_hip_ctx *c = k.c;
  if (k.force != 0 && (!k.wait(k.s, EV_ORDER2) || !k.rec(EV_VOL0, k.s))) return 0;
  const ContArgs ca{c->fb[0].list.as<int>(), c->fb[0].init(), c->maxstep};
  hipExtLaunchKernelGGL(k.vol_fn, dim3((k.np_new + 63) / 64), dim3(64), 0, k.s, nullptr, k.mark(EV_WALK), 0, k.bg,
                        (const Frame *)k.fr, (const unsigned long long *)k.grid, k.g, k.xyz_new, k.pclass,
                        (const int *)k.order_v, k.np_new, k.st, k.S, k.elem_out, k.hit_out, c->filter_steps, k.flag,
                        kXcdRun, ca, k.ma);
  return 1;
}

// ---- tail (main stream): the volume grid's refill, the volume queries' exhaustive fallbacks, the join
static int launch_tail(Call &k) {
  pmmg_hip_ctx *c = k.c;
  hipStream_t s = k.s;
  // the volume seed grid refilled for the next call as soon as the volume kernel is done with it, on its own
  // stream beside the main stream's tail (the fallbacks: latency-bound) and the surface stream's; r06: at the
  // end of the main stream it added ~36 us to a cfg4 call (r05ao: on the surface stream right after the volume
  // kernel it ran behind k_bdy's tail instead)
  const bool refill = k.ng >= kRefillCells;
  if (refill) {
    if (!c->stream_f) HIPCK(c, hipStreamCreateWithFlags(&c->stream_f, hipStreamNonBlocking));
    if (!k.wait(c->stream_f, EV_WALK)) return 0;
    hipExtLaunchKernelGGL(k_fill64, dim3(blocks_for((k.ng + 1) / 2, 2048)), dim3(kBlock), 0, c->stream_f, nullptr,
                          k.mark(EV_FILL), 0, k.grid, k.ng, ~0ULL);
    HIPCK(c, hipGetLastError());
    c->grid_clean_p = c->grid.p;
    c->grid_clean_n = k.ng;
  }
  HIPCK(c, hipGetLastError());
  // exhaustive fallbacks of the volume queries (lists and counts on the
  // device; the surface ones ran on the surface stream after k_bdy): the
  // list's query grid, then the searches, the last of which records EV_JOIN
  launch_fallbacks<4>(k, s, k.mark(EV_JOIN));
  HIPCK(c, hipGetLastError());
  if (!k.wait(s, EV_BDY1) || (refill && !k.wait(s, EV_FILL)) || !k.rec(EV_END, s)) return 0;
  c->pending = true;
  return 1;
}

static int run_device(pmmg_hip_ctx *c, int np_new, const double *xyz_new, const uint8_t *pclass, double *met_out,
                      double *const *fields_out, int *elem_out, int8_t *hit_out, double *rec_out = nullptr,
                      const int *map_src = nullptr) {
  Call k{c, np_new, xyz_new, pclass, elem_out, hit_out, c->bg, c->stream, c->stream2, c->stream2}; // (the rest zero)
  if (!call_slots(k, met_out, fields_out, rec_out, map_src) || !call_scratch(k)) return 0;
  c->ev_done = 0; // from here on the context's events are this call's: none to be read until all are enqueued
  if (!launch_frame_seeds(k)) return 0;
  // A large auto-order call: the launches that do not depend on the order (the input order's surface list, gated
  // on the device flag; the surface seeds) go out before the host waits for the decision, so that after it only
  // the chosen order's kernels are enqueued, the volume kernel first (r06ze: the device idled ~20 us between the
  // seed grid and the volume kernel of an 8-way rank while the host enqueued ~10 launches ahead of it)
  const bool pre = k.force < 0;
  launch_cls(k); // (a forced Morton order has no input-order list)
  if (pre) {
    if (!k.has(EV_ORDER) && !k.rec(EV_ORDER, k.sb)) return 0;
    if (!srf_head(k)) return 0;
    HIPCK(c, hipGetLastError());
    // the decision, written by k_bbox's last block (coherence_final); from here on a forced order
    if (!k.recorded(EV_FRAME)) return 0;
    HIPCK(c, hipEventSynchronize(c->ev[EV_FRAME]));
    const int f = __atomic_load_n(&c->flag_host[0], __ATOMIC_ACQUIRE);
    if (f != 0 && f != 1) {
      set_err(c, "locate_interp: the query order decision did not arrive (%d)", f);
      return 0;
    }
    k.force = f;
  }
  // the chosen order's lists (EV_ORDER2 is waited for only when the order is Morton)
  if (!launch_morton(k)) return 0;
  HIPCK(c, hipGetLastError());
  if (!k.has(EV_ORDER) && !k.rec(EV_ORDER, k.sb)) return 0; // (unless the surface list's last kernel carried it)
  if (k.force != 0 && !k.rec(EV_ORDER2, k.sc)) return 0;    // (sc == sb: the same point)
  if (pre && !launch_vol(k)) return 0;
  if (k.sc != k.sb && k.force != 0 && !k.wait(k.sb, EV_ORDER2)) return 0; // the Morton surface list
  if (!pre && !srf_head(k)) return 0;
  if (k.bg.nt > 0) launch_bdy(k);
  if (!srf_tail(k)) return 0;
  if (!pre && !launch_vol(k)) return 0;
  HIPCK(c, hipGetLastError());
  if (!launch_tail(k)) return 0;
  c->ev_done = k.evs; // what collect_stats may read of this call
  return 1;
}

static int collect_stats(pmmg_hip_ctx *c, pmmg_hip_stats *out) {
  DevStats h;
  int order[2] = {0, 0}; // the call's query order, decided on the device
  HIPCK(c, ctx_d2h(c, order, c->oflag.p, sizeof(order)));
  std::vector<StatPart> parts(kStatParts);
  HIPCK(c, ctx_d2h(c, &h, c->stats.p, sizeof(DevStats)));
  HIPCK(c, ctx_d2h(c, parts.data(), c->stats.as<const DevStats>() + 1, kStatParts * sizeof(StatPart)));
  unsigned long long cnt[kNumCnt] = {0}, steps = 0, stepmax = 0;
  for (const StatPart &pt : parts) {
    for (int j = 0; j < kNumCnt; j++) cnt[j] += pt.cnt[j];
    steps += pt.steps;
    if (pt.stepmax > stepmax) stepmax = pt.stepmax;
  }
  memset(out, 0, sizeof(*out));
  out->nvol = order[0] == 1 ? (int64_t)h.nvol : (int64_t)cnt[kCntVolQueries];
  out->nbdy = h.nbdy;
  out->nvol_walk = (int64_t)cnt[PMMG_HIT_VOL_WALK];
  out->nvol_exhaust = (int64_t)cnt[PMMG_HIT_VOL_EXHAUST];
  out->nvol_closest = (int64_t)cnt[PMMG_HIT_VOL_CLOSEST];
  out->nvol_exact = (int64_t)cnt[kCntExact];
  out->nbdy_face = (int64_t)cnt[PMMG_HIT_BDY_FACE];
  out->nbdy_edge = (int64_t)cnt[PMMG_HIT_BDY_EDGE];
  out->nbdy_vertex = (int64_t)cnt[PMMG_HIT_BDY_VERTEX];
  out->nbdy_wedge = (int64_t)cnt[PMMG_HIT_BDY_WEDGE];
  out->nbdy_cone = (int64_t)cnt[PMMG_HIT_BDY_CONE];
  out->nbdy_exhaust = (int64_t)cnt[PMMG_HIT_BDY_EXHAUST];
  out->nbdy_stale = (int64_t)cnt[PMMG_HIT_BDY_STALE];
  out->nbdy_closest = (int64_t)cnt[PMMG_HIT_BDY_CLOSEST];
  out->steps_total = (int64_t)steps;
  out->stepmax = (int64_t)stepmax;
  out->wave_iters = (int64_t)cnt[kCntWaveIters];
  out->sorted = order[0] == 1;
  out->nvol_noseed = (int64_t)cnt[kCntNoSeed];
  out->nvol_stuck = (int64_t)cnt[kCntStuck];
  out->nvol_limit = (int64_t)cnt[kCntLimit];
  int ad = 0;
  HIPCK(c, ctx_d2h(c, &ad, &c->frame.as<const Frame>()->adaptive, sizeof(int)));
  out->seed_map_axes = ad;
  out->nbdy_fanscan = (int64_t)cnt[kCntFanScan];
  out->nvol_src = (int64_t)cnt[kCntVolSrc];
  out->nbdy_src = (int64_t)cnt[kCntBdySrc];
  // an interval between two events of the call reported on (never an earlier call's record: ev_done)
  auto interval = [c](int a, int b, float *ms) -> int {
    if (!((c->ev_done >> a) & (c->ev_done >> b) & 1u)) {
      set_err(c, "locate_interp: internal: stats interval of events %d and %d, which the call did not both record", a,
              b);
      return 0;
    }
    HIPCK(c, hipEventElapsedTime(ms, c->ev[a], c->ev[b]));
    return 1;
  };
  // the volume stage opens at EV_VOL0 when the call recorded it (Morton order), else right after the seed grid
  const int vol0 = (c->ev_done >> EV_VOL0) & 1u ? EV_VOL0 : EV_PREP;
  if (!interval(EV_START, EV_PREP, &out->ms_prepare) ||
      !interval(EV_SB0, EV_ORDER, &out->ms_sort) || // on the second (and third) stream, concurrent with the seed grid
      !interval(vol0, EV_WALK, &out->ms_vol) ||
      !interval(EV_BDY0, EV_BDY1, &out->ms_bdy) || // on the surface stream, concurrent with the volume kernels
      !interval(EV_WALK, EV_JOIN, &out->ms_fallback) || // the volume queries' exhaustive search (the surface one
      !interval(EV_START, EV_END, &out->ms_total))      // is in ms_bdy)
    return 0;
  out->ms_vol_locate = out->ms_vol; // (one kernel locates and interpolates: the same interval)
  return 1;
}
