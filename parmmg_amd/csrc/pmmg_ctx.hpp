// pmmg_ctx.hpp — the context behind the C-ABI of include/parmmg_hip.h (included by pmmg_hip.hip only): the device
// buffers it owns, its streams, events and settings, the error text, the opening of an entry point, environment
// switches, launch sizes and the size rules of metrics and fields.
#pragma once

#include <hip/hip_runtime.h>
#include <rccl/rccl.h> // ncclComm_t (pmmg_comm.hpp)

#include <math.h>
#include <stdarg.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <algorithm>
#include <thread>
#include <vector>

#include "pmmg_device.hpp"
#include "pmmg_prep.hpp"
#include "pmmg_devbuf.hpp"
#include "pmmg_snapshot.hpp"
#include "pmmg_meshstats.hpp"
#include "pmmg_graph.hpp"
#include "pmmg_contig.hpp"
#include "pmmg_split.hpp"
#include "pmmg_moveifc.hpp"
#include "pmmg_merge.hpp"

using namespace pmmg;

// One family of exhaustive searches (volume or surface queries): what its two
// kernels and its list's query grid work on
struct FbBufs {
  DevBuf list, best;              // the fallback queries, each one's lowest accepting element
  DevBuf nac, cres, part;         // the queries nothing accepted, their closest results and range minima (FbPart)
  DevBuf g_cells, g_cur, g_items; // the list's query grid (FbGridBufs)
  FbInit init() const { return FbInit{best.as<int>()}; }
  FbGridBufs grid() const { return FbGridBufs{g_cells.as<int>(), g_cur.as<int>(), g_items.as<int>()}; }
};

// Every device buffer a context owns, in one base of the context: each frees
// itself (pmmg_devbuf.hpp), and pmmg_hip_destroy resets the whole base at the
// point of its teardown where the streams are idle and still exist.
struct CtxBufs {
  // owned copies for PMMG_HIP_HOST inputs
  DevBuf o_xyz, o_tetv, o_adja, o_triv, o_adjt, o_met, o_rec;
  std::vector<DevBuf> o_f;
  DevBuf o_tet4; // device copy of a host tetv (input of the device adjacency)
  // work buffers
  DevBuf frame, stats, grid, sgrid, order_v, order_b, xq;
  DevBuf cohd;                            // the coherence test's sampled distances (k_bbox)
  DevBuf axh;                             // per-axis histograms of the seed grid map (k_quantize)
  DevBuf bkeys, bkeys2, bvals, bvals2;    // Morton binning: keys and ids, ping-ponged by the radix sort
  DevBuf rs_hist, rs_csum;                // the radix sort's digit table and its scan's chunk sums
  DevBuf cls_cnt;                         // per-block class counts (surface list compaction)
  DevBuf oflag;                           // the coherence test's {sorted, bin_bits} on the device
  DevBuf qmin;                               // tetra quality minimum (pmmg_hip_tetra_qual)
  FbBufs fb[2]; // the exhaustive searches of the volume (0) and of the surface (1) queries
  // host-mode staging
  DevBuf h_xyz, h_cls, h_met, h_elem, h_hit;
  std::vector<DevBuf> h_f;
  SnapCache snap_cache; // the snapshot kernels' scratch (pmmg_snapshot.hip)
  StatsCache stats_cache; // pmmg_hip_qual_histo / pmmg_hip_edge_lengths: edge table, slabs (pmmg_meshstats.hip)
  GraphCache graph_cache; // pmmg_hip_metis_graph: block counts, scan scratch, a built adjacency (pmmg_graph.hip)
  ContigCache contig_cache; // pmmg_hip_part_subgroups / pmmg_hip_fix_contiguity: labels, the table (pmmg_contig.hip)
  SplitCache split_cache; // pmmg_hip_split_groups: the new order, first uses, masks and prefixes (pmmg_split.hip)
  MoveCache move_cache; // pmmg_hip_ifc_seed / _ifc_layers / _remap_colors: keys, copies of a layer (pmmg_moveifc.hip)
  MergeCache merge_cache; // pmmg_hip_merge_groups: the tables, lowest entries, counts and prefixes (pmmg_merge.hip)
  struct Kept { // a carry-over slot (see pmmg_hip_ctx::carry_slot)
    DevBuf xyz, met;
    std::vector<DevBuf> f;
    int np = 0, met_size = 0;
    std::vector<int> fsize;
    bool valid = false;
  };
  std::vector<Kept> kept;
  DevBuf carry_dsrc, carry_need, carry_ids, carry_cnt, carry_rows, carry_bc;
  DevBuf map_own;  // the copy of a PMMG_HIP_HOST map
  DevBuf map_need; // the call's volume / surface queries without a mapped start (k_map_count)
  DevBuf start_tab; // the background's start tables (see pmmg_hip_ctx::map_src)
  DevBuf ag_send, ag_recv, ag_off, ag_chk; // the all-gather's buffers (ag_chk: its agreement, ag_agree)
};

enum {
  EV_START, EV_FRAME, EV_PREP, EV_ORDER, EV_VOL0, EV_WALK, EV_JOIN, EV_END, EV_BDY0, EV_BDY1, EV_RESET,
  EV_SB0, EV_ORDER2, EV_FILL, EV_COUNT
};

struct pmmg_hip_ctx : CtxBufs {
  int device = 0;
  int options = 0;
  hipStream_t stream = nullptr;
  hipStream_t stream2 = nullptr; // surface branch, concurrent with the volume walk
  hipStream_t stream3 = nullptr; // Morton binning of a call that may take that order (created at the first such
                                 // call, not with the context: a context that never bins keeps to two streams),
                                 // beside the input order's surface list on stream2
  hipStream_t stream_f = nullptr; // a large call's seed-grid refill, right after the volume kernel, beside the
                                  // main stream's tail (created at the first such call)
  char err[512] = {0};
  Bg bg{};
  int met_size = 0;
  int nfield = 0;
  std::vector<int> fsize;
  std::vector<const double *> fin;
  const double *met = nullptr;
  const double *rec = nullptr; // packed per-vertex solution records (set_solutions_packed), else null
  int rstride = 0;             // their stride in doubles
  // the seed grids left clean by the previous call (its last kernels refill
  // them while the other stream finishes): k_reset skips what is clean
  void *grid_clean_p = nullptr, *sgrid_clean_p = nullptr;
  long long grid_clean_n = 0, sgrid_clean_n = 0;
  hipEvent_t ev[EV_COUNT] = {};
  bool pending = false;
  // host-mode transfers: two pinned staging buffers, filled / drained by a
  // small pool of host threads while the DMA engine moves the other one
  void *stage[2] = {nullptr, nullptr};
  void *stage_dev[2] = {nullptr, nullptr}; // their device addresses (kernel downloads)
  hipEvent_t stage_ev[2] = {};
  int stage_i = 0;
  struct Pool *pool = nullptr;
  int edge_hash = 1;      // the edge table's slot: 1 a run of slots per low vertex first, 0 a mix of the whole
                          // key (PMMG_HIP_EDGEHASH=0; cfg4: 31.0 against 56.0 ms)
  // host mode: the device-built background (adjacency, boundary trias) runs
  // on `stream` in a host thread while set_solutions' uploads go through
  // `cstream` (the DMA engine works beside the snapshot kernels); every other
  // entry point joins it first (snap_join)
  hipStream_t cstream = nullptr;
  std::thread snap;
  int snap_ok = 1;
  int verbose = 0; // PMMG_HIP_VERBOSE: host-mode transfer timings on stderr
  int tpc = 8;        // background tetra per volume seed cell (PMMG_HIP_TPC)
  int pack_passes = 0; // packed records gathered in 1 or 2 passes over the record (PMMG_HIP_PACKPASS; 0: by size)
  unsigned ev_done = 0; // the events the last call recorded, bit by bit (Call::evs; collect_stats reads no other)
  int *flag_host = nullptr;     // (pinned, coherent: k_bbox's last block writes the decision here too)
  int *flag_host_dev = nullptr; // (its device address)
  int srf_g = 0;         // test-only PMMG_HIP_SRFG: the surface seed grid's cells per axis (1: one seed for all)
  int srf_mult = 8;      // the surface seed grid has srf_mult * nt / 2 cells (PMMG_HIP_SRFMULT; r03r at cfg4: 1 /
                         // 8 / 32 -> 7.4 / 3.9 / 2.7 steps per surface point, surface branch 0.446 / 0.403 /
                         // 0.399 ms: a surface grid sized like a volume grid left ~33 trias per occupied cell)
  int bin_bits = kBinBitsCoherent; // Morton bits per axis of the binning keys when the order is forced (1..7,
                                    // PMMG_HIP_BINBITS; auto mode: the coherence test picks)
  int maxstep = 1024; // longer walks go to the exhaustive kernels (PMMG_HIP_MAXSTEP; the reference caps at ne).
                      // r05: 4096 -> 1024; a walk that long cycles along a concave boundary (carried cfg4
                      // iteration: 2644 queries at the cap, all then accepted by the exhaustive search; the
                      // longest legitimate walk seen is 302 steps, cfgG)
  int fanmax = kFanMax;    // cone fans longer than this take the O(nt) scan (test-only PMMG_HIP_FANMAX)
  // carry-over (pmmg_hip_keep / pmmg_hip_carry_over): kept[slot] holds the new
  // points and written rows of a host-mode call; an armed carry (carry_slot
  // >= 0) feeds the next host-mode set_background / set_solutions from it
  int last_host_np = 0, last_host_met = 0; // the last host-mode locate_interp (what pmmg_hip_keep keeps)
  std::vector<int> last_host_fsize;
  int carry_slot = -1, carry_np = 0;
  bool carry_bg = false;       // set_background took its vertices from the carry
  std::vector<int> carry_src;  // next vertex i+1 = kept point carry_src[i] (0: host row); empty: identity
  int64_t bytes_up = 0; // host -> device bytes of host-mode calls (pmmg_hip_bytes_up)
  // point map (pmmg_hip_set_point_map): map_src != null arms the next locate_interp(_rec) of map_np new
  // points, which consumes it.  start_tab: the background's start tables, start_tet[np] then start_tri[np]
  // (k_start_tet / k_start_tri), built at the first mapped call or pmmg_hip_start_elements on a background
  // and kept until the next set_background* or pmmg_hip_release_scratch
  const int *map_src = nullptr;
  int map_np = 0;
  bool start_valid = false;
  // pmmg_hip_locate_interp_groups: lanes[j] is lane j (same device and
  // options, created at the first groups call); lane 0 enqueues on this
  // context's own streams (no extra hardware queue) but has its own state, so
  // a groups call leaves this context's background and solutions as they were.
  // Every other lane has one stream, its surface branch on its main stream.
  std::vector<pmmg_hip_ctx *> lanes;
  bool borrowed_streams = false; // a lane 0: stream / stream2 belong to its parent
  // the split of a group over the node's GPUs (pmmg_comm.hpp): an RCCL
  // communicator, owned (pmmg_hip_comm_init) or the caller's (attach)
  ncclComm_t comm = nullptr;
  bool comm_owned = false;
  int comm_rank = 0, comm_size = 0;
  // PMMG_HIP_GROUP_LANES: most lanes of a groups call (r05k, 10 cfg2-size groups, 4 hardware queues: 4 / 5 /
  // 8 / 10 lanes 0.096 / 0.083 / 0.092 / 0.095 ms per group — 5 lanes take 2 groups each, 4 take 3, 3, 2, 2;
  // more hardware queues made it slower: 8 queues, 5 lanes 0.127; r04i: 1 / 2 lanes 0.165 / 0.125)
  // r06 (profiles/r06m, 3 rounds each, after a fresh start / after a large call in the process): 5 lanes of
  // 2 streams 0.090 / 0.106 ms per group, 4 x 2 0.079 / 0.091, 4 x 1 0.096 / 0.103, 5 x 1 0.096 / 0.085,
  // 3 x 1 0.081 / 0.082.  The hardware has 4 queues (GPU_MAX_HW_QUEUES): lane 0 on this context's two
  // streams plus two lanes of one stream each is 4 streams, one per queue whatever queues earlier streams of
  // the process left (a new stream takes the least used queue, ties broken in an order that changes from
  // process to process: with 10 streams two busy lanes shared a queue in some processes and not in others —
  // the r05 "slowdown after a large call")
  int group_lanes = 3;
  struct Pool *lane_pool = nullptr; // host threads enqueueing the other lanes' groups
  int filter_steps = 64; // step cap of the fp32 filter walk (then the exact fp64 walk continues from where it
                         // stopped: a query the filter misjudges hands over early instead of cycling through a
                         // 4-entry history for up to maxstep steps); test-only PMMG_HIP_FILTER_STEPS=0 sends every
                         // volume query to the exact walk
};

static void set_err(pmmg_hip_ctx *c, const char *fmt, ...) {
  if (!c) return;
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(c->err, sizeof(c->err), fmt, ap);
  va_end(ap);
  fprintf(stderr, "[parmmg_hip] %s\n", c->err);
}

#define HIPCK(ctx, expr)                                                                             \
  do {                                                                                               \
    hipError_t e_ = (expr);                                                                          \
    if (e_ != hipSuccess) {                                                                          \
      set_err((ctx), "%s failed: %s (%s:%d)", #expr, hipGetErrorString(e_), __FILE__, __LINE__);   \
      return 0;                                                                                      \
    }                                                                                                \
  } while (0)

// Device -> host reads of a context's small state on its own stream (r06):
// a synchronous hipMemcpy goes through the device's null stream, whose queue
// user — created at the first such copy — shifted the hardware queues the
// group lanes' streams were later given (the groups call
// 25 % slower after any earlier call in the process; tools/groups_probe.py,
// profiles/r06f).
static hipError_t ctx_d2h(pmmg_hip_ctx *c, void *dst, const void *src, size_t n) {
  hipError_t e = hipMemcpyAsync(dst, src, n, hipMemcpyDeviceToHost, c->stream);
  return e != hipSuccess ? e : hipStreamSynchronize(c->stream);
}

static int ensure(pmmg_hip_ctx *c, DevBuf &b, size_t bytes) {
  const hipError_t e = b.ensure(bytes);
  if (e != hipSuccess) {
    set_err(c, "hipMalloc(&b.p, bytes) failed: %s (%s:%d)", hipGetErrorString(e), __FILE__, __LINE__);
    return 0;
  }
  return 1;
}

// the host-mode copy stream, created at the first host-mode upload (a
// device-mode context, and every group lane, keeps to two streams: the
// process has few hardware queues, GPU_MAX_HW_QUEUES = 4 by default, and
// streams beyond them share one)
static int copy_stream(pmmg_hip_ctx *c) {
  if (!c->cstream) HIPCK(c, hipStreamCreateWithFlags(&c->cstream, hipStreamNonBlocking));
  return 1;
}

static int env_int(const char *name, int def) { // positive values only
  const char *e = getenv(name);
  if (e && atoi(e) > 0) return atoi(e);
  return def;
}
// switches whose 0 (or -1) is a setting of its own (env_int reads 0 as unset)
static int env_int_any(const char *name, int def) {
  const char *e = getenv(name);
  if (!e || !*e) return def;
  char *end = nullptr;
  const long v = strtol(e, &end, 10);
  return (end && *end == 0) ? (int)v : def;
}

// a background whose snapshot failed is dropped: its tet8 adjacency or
// boundary trias may be partly written, so no later call may walk it (the
// 'no background set' guard then fails them until set_background succeeds)
static void invalidate_bg(pmmg_hip_ctx *c) {
  c->bg.ne = c->bg.nt = c->bg.np = 0;
  c->bg.tetv = c->bg.adja = nullptr;
  c->bg.triv = c->bg.adjt = nullptr;
  c->bg.xyz = nullptr;
  c->start_valid = false;
}

// wait for a deferred device snapshot (host-mode set_background); 0 if it failed
static int snap_join(pmmg_hip_ctx *c) {
  if (c->snap.joinable()) c->snap.join();
  if (!c->snap_ok) {
    c->snap_ok = 1; // reported once, by the call that joined it
    invalidate_bg(c);
    return 0;
  }
  return 1;
}

// what opens an entry point that works on the device: the context's device
// made current, then a deferred snapshot joined
static int enter(pmmg_hip_ctx *c) {
  if (!c) return 0;
  HIPCK(c, hipSetDevice(c->device));
  if (!snap_join(c)) return 0;
  return 1;
}

// share != NULL: a group lane that enqueues on share's two streams (its
// own buffers, events and state; the streams are not destroyed with it)
static pmmg_hip_ctx *create_ctx(int device, int options, pmmg_hip_ctx *share = nullptr) {
  int n = pmmg_hip_device_count();
  if (n <= 0 || device < 0 || device >= n) {
    fprintf(stderr, "[parmmg_hip] no HIP device %d (visible: %d)\n", device, n);
    return nullptr;
  }
  pmmg_hip_ctx *c = new pmmg_hip_ctx();
  c->device = device;
  c->options = options;
  if (share) {
    c->stream = share->stream;
    c->stream2 = share->stream2;
    c->borrowed_streams = true;
  }
  if (hipSetDevice(device) != hipSuccess ||
      (!share && (hipStreamCreateWithFlags(&c->stream, hipStreamNonBlocking) != hipSuccess ||
                  hipStreamCreateWithFlags(&c->stream2, hipStreamNonBlocking) != hipSuccess))) {
    fprintf(stderr, "[parmmg_hip] cannot initialise device %d\n", device);
    delete c;
    return nullptr;
  }
  for (int i = 0; i < EV_COUNT; i++) (void)hipEventCreateWithFlags(&c->ev[i], hipEventDefault);
  // documented options, each clamped to its valid range
  c->tpc = std::min(4096, env_int("PMMG_HIP_TPC", c->tpc));
  c->srf_mult = std::min(4096, env_int("PMMG_HIP_SRFMULT", c->srf_mult));
  c->bin_bits = std::min(7, env_int("PMMG_HIP_BINBITS", c->bin_bits));
  c->verbose = env_int("PMMG_HIP_VERBOSE", 0);
  c->edge_hash = env_int_any("PMMG_HIP_EDGEHASH", 1) == 0 ? 0 : 1;
  c->maxstep = env_int("PMMG_HIP_MAXSTEP", c->maxstep);
  c->group_lanes = std::min(16, env_int("PMMG_HIP_GROUP_LANES", c->group_lanes));
  // test-only path selection (tests/test_gpu_hits.py, tests/test_gpu_parity.py)
  c->fanmax = env_int("PMMG_HIP_FANMAX", c->fanmax);
  c->srf_g = std::min(1024, env_int("PMMG_HIP_SRFG", 0));
  c->pack_passes = std::max(0, std::min(2, env_int("PMMG_HIP_PACKPASS", c->pack_passes))); // packed: gather passes
  c->bg.fanmax = c->fanmax; // every kernel's Bg copy carries it
  c->filter_steps = c->filter_steps < c->maxstep ? c->filter_steps : c->maxstep;
  if (const char *e = getenv("PMMG_HIP_FILTER_STEPS"))
    if (*e && atoi(e) >= 0) c->filter_steps = atoi(e);
  return c;
}

// the sizes a metric (none, iso, aniso) and a field (MMG5_Scalar / MMG5_Vector / MMG5_Tensor) may have
static bool valid_met_size(int n) { return n == 0 || n == 1 || n == 6; }
static bool valid_field_size(int n) { return n == 1 || n == 3 || n == 6; }

static int grid_dim(long long n, int per_cell, int gmax) {
  double g = cbrt((double)n / (double)per_cell);
  int gi = (int)g;
  if (gi < 1) gi = 1;
  if (gi > gmax) gi = gmax;
  return gi;
}

static int blocks_for(long long n, int cap) {
  long long b = (n + kBlock - 1) / kBlock;
  if (b < 1) b = 1;
  if (b > cap) b = cap;
  return (int)b;
}
