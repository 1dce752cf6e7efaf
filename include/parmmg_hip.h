/*
 * parmmg_hip.h — C-ABI of the MI355X (gfx950) old->new mesh transfer module.
 *
 * This is the drop-in boundary for ParMmg's metric/field interpolation step.
 * It replaces, per group, the body of
 *
 *   int PMMG_interpMetricsAndFields(PMMG_pParMesh parmesh, int *permNodGlob)
 *       reference: src/interpmesh_pmmg.c:663-741, prototype src/parmmg.h:472,
 *       called once per remeshing iteration from src/libparmmg1.c:829
 *
 * and, below it, the static per-group worker
 *
 *   PMMG_interpMetricsAndFields_mesh(...)      src/interpmesh_pmmg.c:477-649
 *
 * together with everything it reaches: PMMG_locatePointVol / _Bdy
 * (src/locate_pmmg.c:786-883, :587-723), the barycentric evaluation
 * (src/barycoord_pmmg.c) and the interpolators bound through the
 * PMMG_interp{2,3,4}bar function pointers (src/parmmgexterns.c:4-6,
 * bound by PMMG_setfunc src/libparmmg_tools.c:595-612).
 *
 * Conventions (all entry points):
 *  - Plain pointers and sizes only; no torch or HIP types in signatures.
 *  - Return 1 on success, 0 on failure: the internal ParMmg convention of
 *    PMMG_interpMetricsAndFields (NOT the public PMMG_SUCCESS=0 convention).
 *  - Arrays are "row r = entity r+1": ParMmg entities are 1-based, entry 0 is
 *    unused.  A host shim passes e.g. `met->m + met->size` for the metric and
 *    `mesh->adja + 1` for the tetra adjacency, so no copy is needed for those.
 *  - Entity ids stored INSIDE arrays keep the reference encoding: vertex ids
 *    in tetv/triv are 1-based, adja holds 4*k'+i' (0 = boundary face,
 *    src/locate_pmmg.c:821), adjt holds 3*k'+i' (0 = surface border,
 *    src/locate_pmmg.c:635).
 *  - `where` = PMMG_HIP_HOST: pointers are host memory, calls copy (through
 *    pinned staging buffers of the context) and are synchronous.  `where` = PMMG_HIP_DEVICE: pointers are device memory on
 *    the context's device; set_* calls only record the pointers (no copy) and
 *    pmmg_hip_locate_interp only enqueues work on the context's streams (no
 *    host synchronisation inside the call: every decision — query order,
 *    fallback launches — is taken on the device); use pmmg_hip_sync before
 *    reading results or stats.
 *  - The module is reentrant per context (the reference is not: it uses
 *    static warning flags and global function pointers).
 */
#ifndef PARMMG_HIP_H
#define PARMMG_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define PMMG_HIP_HOST   0
#define PMMG_HIP_DEVICE 1

/* Per-point classification supplied by the caller (the host shim derives it
 * from Mmg tags in the reference's visitation loop, src/interpmesh_pmmg.c:535-550). */
#define PMMG_PT_SKIP 0   /* invalid, MG_REQ (copied by PMMG_copyMetricsAndFields_point) or unreferenced */
#define PMMG_PT_VOL  1   /* volume point   -> PMMG_locatePointVol path */
#define PMMG_PT_BDY  2   /* MG_BDY point   -> PMMG_locatePointBdy path */

/* Located-element kind written to hit_out (diagnostics + parity checking). */
#define PMMG_HIT_NONE         0  /* not processed (PMMG_PT_SKIP) */
#define PMMG_HIT_VOL_WALK     1  /* adjacency walk accepted the tetra          locate_pmmg.c:814-815 */
#define PMMG_HIT_VOL_EXHAUST  2  /* exhaustive scan: lowest-index accepted      locate_pmmg.c:743-762 */
#define PMMG_HIT_VOL_CLOSEST  3  /* not located: closest tetra, nearest vertex  locate_pmmg.c:764-767 */
#define PMMG_HIT_BDY_FACE     4  /* tria walk accepted, interior of the tria    locate_pmmg.c:624-627 */
#define PMMG_HIT_BDY_EDGE     5  /* tria walk accepted, on an edge (isBorder)   barycoord_pmmg.c:109-120 */
#define PMMG_HIT_BDY_VERTEX   6  /* tria walk accepted, at a vertex (isBorder)  barycoord_pmmg.c:109-120 */
#define PMMG_HIT_BDY_WEDGE    7  /* edge shadow wedge                           locate_pmmg.c:643-649 */
#define PMMG_HIT_BDY_CONE     8  /* vertex shadow cone                          locate_pmmg.c:651-657 */
#define PMMG_HIT_BDY_EXHAUST  9  /* exhaustive tria scan: lowest-index accepted locate_pmmg.c:483-503 */
#define PMMG_HIT_BDY_STALE   10  /* not located, re-evaluation accepted         locate_pmmg.c:505-509 */
#define PMMG_HIT_BDY_CLOSEST 11  /* not located: closest tria, nearest vertex   locate_pmmg.c:511,681 */

#define PMMG_HIT_CODE(h) ((h) & 15)
#define PMMG_HIT_LOC(h)  (((h) >> 4) & 3)

typedef struct pmmg_hip_ctx pmmg_hip_ctx;

/* Counters of one pmmg_hip_locate_interp call (the reference's debug-only
 * PMMG_locateStats, src/locate_pmmg.h:45-50, plus per-phase device times). */
typedef struct {
  int64_t nvol;          /* volume queries */
  int64_t nbdy;          /* surface queries */
  int64_t nvol_walk, nvol_exhaust, nvol_closest;
  int64_t nvol_exact;    /* volume queries the fp32 filter walk handed to the exact (fp64) walk */
  int64_t nbdy_face, nbdy_edge, nbdy_vertex, nbdy_wedge, nbdy_cone;
  int64_t nbdy_exhaust, nbdy_stale, nbdy_closest;
  int64_t steps_total;   /* walk steps, volume + surface */
  int64_t stepmax;
  int64_t wave_iters;    /* sum over wavefronts of their longest walk (lockstep cost; steps_total /
                            (64 * wave_iters) = lockstep efficiency) */
  int64_t sorted;        /* 1 if the queries were Morton-binned, 0 if processed in input order */
  /* device time in milliseconds, measured with HIP events on the context stream */
  float ms_prepare;      /* bbox, seed grids, input-order coherence test */
  float ms_sort;         /* query order: Morton binning, or stable class compaction */
  float ms_vol;          /* volume locate + interpolate kernels */
  float ms_bdy;          /* surface branch: locate + interpolate, its exhaustive / closest kernels */
  float ms_fallback;     /* exhaustive / closest kernels of the volume queries */
  float ms_total;        /* whole call, first to last event */
  float ms_vol_locate;   /* the volume walk kernel alone (part of ms_vol) */
  int64_t nvol_noseed;   /* volume queries with no seed within 6 seed-grid cells: walked from the lowest
                            in-use tetra the grid sampled */
  int64_t nvol_stuck;    /* exact volume walks stuck (no eligible neighbour) -> exhaustive */
  int64_t nvol_limit;    /* exact volume walks stopped at maxstep -> exhaustive */
  int64_t seed_map_axes; /* bit d: axis d of the volume seed grid followed the vertex quantiles */
  int64_t nbdy_fanscan;  /* surface queries whose cone test scanned every tria for a vertex's ball (its fan
                            open, non-manifold or longer than 64: e.g. at a halo shard's cut) */
  int64_t nvol_src;      /* volume queries whose walk began from the point map (pmmg_hip_set_point_map) */
  int64_t nbdy_src;      /* surface queries whose tria walk began from the point map */
  int64_t reserved[4];   /* zero; room for later counters without changing the struct's size */
} pmmg_hip_stats;

/* ABI of this header (r06): a shim built against it checks, once at load,
 *     pmmg_hip_abi_version() == PMMG_HIP_ABI_VERSION
 *     pmmg_hip_stats_size()  == sizeof(pmmg_hip_stats)
 * and refuses a library that differs: the library writes a whole
 * pmmg_hip_stats into the caller's struct (round 5 appended nbdy_fanscan, so a
 * shim built against the round-4 header would have been overrun by 8 bytes).
 * Entry points added since (the group split, the interface displacement) leave the version as it is: no
 * existing signature or struct changed, so a shim built against the earlier
 * header of version 6 runs unchanged against this library; a shim that needs a
 * later entry point finds out from the symbol itself. */
#define PMMG_HIP_ABI_VERSION 6
int pmmg_hip_abi_version(void);
int64_t pmmg_hip_stats_size(void);

/* Options (bit flags) for pmmg_hip_create.  Default: Morton-bin the queries
 * unless a sampled test on the device finds the input numbering already
 * spatially coherent (3 in 4 consecutive points closer than 4 mean
 * spacings), and groups of fewer than 2^20 new points keep their input order. */
#define PMMG_HIP_OPT_NOSORT 1   /* always process queries in input order */
#define PMMG_HIP_OPT_SORT   2   /* always Morton-bin the queries */

/* Create a context on HIP device `device`.  Returns NULL on failure. */
pmmg_hip_ctx *pmmg_hip_create(int device, int options);
void pmmg_hip_destroy(pmmg_hip_ctx *ctx);

/* Background (pre-remesh) mesh of one group: the reference's oldMesh after
 * PMMG_update_oldGrps (src/grpsplit_pmmg.c:1224).
 *   np    vertices, xyz[3*np]        (MMG5_Point.c, packed)
 *   ne    tetrahedra, tetv[4*ne]     (MMG5_Tetra.v, packed), adja[4*ne] (= &mesh->adja[1])
 *   nt    boundary trias, triv[3*nt] (MMG5_Tria.v, packed),  adjt[3*nt] (= &mesh->adjt[1])
 *   hausd surface distance tolerance (oldMesh->info.hausd, src/locate_pmmg.c:253,315,363)
 * What PMMG_create_oldGrp derives from the connectivity (src/grpsplit_pmmg.c:
 * 350-415) may instead be built on the device:
 *   adja == NULL            the tetra adjacency (MMG3D_hashTetra's result)
 *   triv == NULL, nt < 0    the boundary trias, in (tetra, face) order oriented
 *                           by MMG5_idir, and their adjacency (MMG5_chkBdryTria
 *                           + MMG3D_hashTria for a single-material old mesh
 *                           without input trias)
 *   adjt == NULL, triv set  the tria adjacency (MMG3D_hashTria)
 * In host mode this also spares the PCIe upload of those arrays (the
 * adjacency is as large as the connectivity).  nt may be 0 (then no
 * PMMG_PT_BDY query may be submitted). */
int pmmg_hip_set_background(pmmg_hip_ctx *ctx, int np, const double *xyz,
                            int ne, const int *tetv, const int *adja,
                            int nt, const int *triv, const int *adjt,
                            double hausd, int where);

/* Same background with the tetrahedra as packed 32-byte records
 *   tet8[8*ne] = {v0, v1, v2, v3, adja0, adja1, adja2, adja3} per tetra
 * (MMG5_Tetra.v followed by the tetra's 4 adja codes 4*k+i).  This is the
 * module's preferred HBM layout: a walk step reads one record (one cache
 * line) instead of a tetv row plus an adja row.  A host shim builds it in the
 * same pass that packs MMG5_Tetra.v.  In device mode tet8
 * must be 16-byte aligned. */
int pmmg_hip_set_background_tet8(pmmg_hip_ctx *ctx, int np, const double *xyz,
                                 int ne, const int *tet8,
                                 int nt, const int *triv, const int *adjt,
                                 double hausd, int where);

/* Background solutions: the metric (met_size 0 = none, 1 = iso, 6 = aniso,
 * storage m11,m12,m13,m22,m23,m33 as MMG5 stores it) and nfield fields of
 * size field_size[j] (1, 3 or 6; size 6 fields use the inverse-tensor
 * interpolation, src/interpmesh_pmmg.c:582-593,623-634).
 * met[met_size*np], fields[j][field_size[j]*np] (= sol->m + sol->size).
 * Device-mode size-6 arrays must be 16-byte aligned. */
int pmmg_hip_set_solutions(pmmg_hip_ctx *ctx, int met_size, const double *met,
                           int nfield, const int *field_size,
                           const double *const *fields, int where);

/* Locate every new point with pclass != PMMG_PT_SKIP and interpolate the
 * metric and fields into it.
 *   np_new         new-mesh vertices; xyz_new[3*np_new], pclass[np_new]
 *   met_out        [met_size*np_new] (may be NULL iff met_size == 0)
 *   fields_out[j]  [field_size[j]*np_new]
 *   elem_out       [np_new] located tetra/tria id (1-based), may be NULL
 *   hit_out        [np_new] PMMG_HIT_* code in bits 0-3; for EDGE / WEDGE the
 *                  local edge, for VERTEX / CONE the local vertex of the tria
 *                  in bits 4-5 (PMMG_HIT_CODE / PMMG_HIT_LOC); may be NULL
 *   stats          may be NULL (with PMMG_HIP_DEVICE it is filled at pmmg_hip_sync)
 * Rows of points that are skipped, and rows whose tensor inversion fails
 * (MMG5_invmat, src/interpmesh_pmmg.c:258-267), are left untouched, as in the
 * reference. */
int pmmg_hip_locate_interp(pmmg_hip_ctx *ctx, int np_new, const double *xyz_new,
                           const uint8_t *pclass, double *met_out,
                           double *const *fields_out, int *elem_out,
                           int8_t *hit_out, pmmg_hip_stats *stats, int where);

/* ---- Point map (Mmg's USE_POINTMAP) -------------------------------------------
 * With USE_POINTMAP Mmg gives every new point the old-mesh vertex it descends
 * from (MMG5_Point.src, src/libparmmg1.c:667-669); PMMG_locate_setStart
 * (src/locate_pmmg.c:931-986) turns it into a start element per point — the
 * first tria holding the source vertex for a boundary point, the first tetra
 * for a volume point — and the walks begin there (src/interpmesh_pmmg.c:
 * 552-554, 602-604) instead of at the previous point's element.
 *
 * Arms the next pmmg_hip_locate_interp / pmmg_hip_locate_interp_rec on this context:
 * src[np_new], src[i] = 1-based background vertex the new point i+1 descends from
 * (MMG5_Point.src under USE_POINTMAP), 0 = unknown.  Ids outside [1, np] of the
 * background count as 0.  Consumed by that call; a call whose np_new differs
 * returns 0 and disarms.  where = PMMG_HIP_HOST copies src (counted in bytes_up),
 * PMMG_HIP_DEVICE records the pointer (must stay valid until the call completes).
 *
 * In the armed call a PMMG_PT_VOL point whose source has a start tetra begins
 * its walk there, a PMMG_PT_BDY point whose source has a start tria begins
 * its tria walk there (stats: nvol_src, nbdy_src); every other point — source
 * unknown, or a surface point whose source is an interior vertex — takes the
 * module's seed grids as in a call without a map, and a seed grid no query
 * needs is not filled.  Results obey the same contract as without a map: the
 * element of a point inside exactly one element does not depend on the start.
 * pmmg_hip_locate_interp_groups neither consumes nor sees an armed map; the
 * map refers to the background as set (an armed carry-over may coexist). */
int pmmg_hip_set_point_map(pmmg_hip_ctx *ctx, int np_new, const int *src, int where);

/* Downloads / copies the background's start tables (either may be NULL); builds them if needed.
 * start_tet[np] / start_tri[np]: per background vertex the lowest-index in-use
 * tetra (v[0] > 0) / boundary tria holding it, 0 when there is none — what
 * PMMG_locate_setStart's ascending loops find.  The tables are built at the
 * first armed call (or this call) on a background, on the device, after a
 * device-built boundary is finished; they are kept until the next
 * pmmg_hip_set_background* and freed by pmmg_hip_release_scratch (the next
 * armed call builds them again). */
int pmmg_hip_start_elements(pmmg_hip_ctx *ctx, int *start_tet, int *start_tri, int where);

/* Wait for all work queued on the context (groups calls included); fills the
 * stats of the last PMMG_HIP_DEVICE pmmg_hip_locate_interp call.  Returns 1/0. */
int pmmg_hip_sync(pmmg_hip_ctx *ctx, pmmg_hip_stats *stats);

/* ---- Carry-over of the new mesh into the next iteration ----------------------
 * ParMmg's next iteration takes the adapted group as its old group
 * (src/libparmmg1.c:653 -> PMMG_update_oldGrps, src/grpsplit_pmmg.c:1224-1248):
 * its vertices are the points this step located and its solutions the rows
 * this step wrote.  After a PMMG_HIP_HOST pmmg_hip_locate_interp they are
 * still in HBM:
 *   pmmg_hip_keep(ctx, slot)    keeps that call's new points and written rows
 *                               in `slot` (0..1023; no copy)
 *   pmmg_hip_carry_over(ctx, slot, np, src)
 *                               arms the next PMMG_HIP_HOST set_background +
 *                               set_solutions: vertex i+1 of the new background
 *                               is kept point src[i] (1-based; NULL: the
 *                               identity, np = the kept count).  Those calls
 *                               still take the full host arrays, but upload
 *                               only the vertices with src[i] == 0 (moved in,
 *                               e.g. by load balancing) and the solution rows
 *                               the step did not write (skipped points, whose
 *                               values the caller copies on the host, and
 *                               MMG5_invmat failures); a metric / field whose
 *                               size differs from the kept one goes up whole.
 * pmmg_hip_carry_over(ctx, slot, 0, NULL) drops the slot and frees its device
 * buffers.  A carry consumes its slot (keep again for the next iteration);
 * any failure of the armed set_background / set_solutions disarms it, and an
 * armed carry rejects pmmg_hip_set_solutions_packed and PMMG_HIP_DEVICE
 * calls.  The kept rows must not have been changed on the host in between;
 * the connectivity always comes from the host.  Both return 1/0. */
int pmmg_hip_keep(pmmg_hip_ctx *ctx, int slot);
int pmmg_hip_carry_over(pmmg_hip_ctx *ctx, int slot, int np, const int *src);

/* Host -> device bytes moved by host-mode calls since the last reset. */
int64_t pmmg_hip_bytes_up(pmmg_hip_ctx *ctx, int reset);

/* Free the context's reusable scratch: the snapshot builders' buckets (12 B x
 * 4 x ne for the adjacency: ~4.8 GB at 101M tetra), the Morton binning's
 * second key / value arrays and digit tables, the point map's start tables
 * (pmmg_hip_start_elements), the scratch of pmmg_hip_qual_histo /
 * pmmg_hip_edge_lengths (the edge table, 12 B x (12 np + 2 nskip) slots: ~2.9 GB
 * at cfg4's adapted mesh of 20.35M points; one ownership byte per tetra; the
 * per-block slabs, under 1 MB), and the group lanes (contexts
 * of their own, re-created by the next groups call).  The next call that
 * needs any of them allocates it again.  Waits for the context's work first.
 * The background, solutions, kept slots and seed grids stay.  Returns 1/0. */
int pmmg_hip_release_scratch(pmmg_hip_ctx *ctx);

/* ---- Many groups in one call ------------------------------------------------
 * ParMmg transfers group by group (the loop of src/interpmesh_pmmg.c:690 over
 * up to PMMG_REMESHER_NGRPS_MAX = 100 groups per rank, src/parmmg.h:212);
 * a group of a few hundred thousand points is launch-bound on one stream.  One
 * group: the arguments of pmmg_hip_set_background(_tet8) +
 * pmmg_hip_set_solutions + pmmg_hip_locate_interp, all PMMG_HIP_DEVICE
 * pointers (same alignment rules). */
typedef struct {
  /* background (old group): tet8 != NULL selects packed records, else tetv +
   * adja (adja NULL: adjacency built on the device, which synchronises); nt <
   * 0 with triv NULL: boundary trias built on the device (synchronises) */
  int np, ne, nt;
  const double *xyz;
  const int *tet8;
  const int *tetv, *adja;
  const int *triv, *adjt;
  double hausd;
  /* solutions at the background vertices */
  int met_size;
  const double *met;
  int nfield;
  const int *field_size;
  const double *const *fields;
  /* the new group's points and outputs */
  int np_new;
  const double *xyz_new;
  const uint8_t *pclass;
  double *met_out;
  double *const *fields_out;
  int *elem_out;
  int8_t *hit_out;
} pmmg_hip_group;

/* Enqueue the transfer of ngroup groups: group i runs on lane i % L of the
 * context (L = ceil(ngroup / rounds), rounds = ceil(ngroup / Lmax), Lmax =
 * PMMG_HIP_GROUP_LANES, default 5: every lane gets the same number of groups
 * give or take one, in the fewest rounds; a lane is a
 * pair of streams with its own work buffers, so the groups of different lanes
 * overlap on the device).  stats == NULL: the call only enqueues (nothing is
 * read back; use pmmg_hip_sync before reading outputs).  stats != NULL: the
 * call waits after each round of L groups and returns the counters summed
 * over all groups (ms_* summed as well, stepmax the largest, sorted the
 * number of groups whose queries were Morton-binned).  Results are identical to one
 * pmmg_hip_locate_interp per group.  The lanes are contexts of their own
 * (lane 0 enqueues on ctx's streams): ctx's background, solutions and armed
 * carry-over are left as they were.  Returns 1 if every group was enqueued
 * (and, with stats, completed), 0 at the first invalid group (the error names
 * its index; groups before it are enqueued). */
int pmmg_hip_locate_interp_groups(pmmg_hip_ctx *ctx, int ngroup, const pmmg_hip_group *groups,
                                  pmmg_hip_stats *stats);

/* ---- Background snapshot on the device -------------------------------------
 * ParMmg rebuilds the background's derived arrays on the host every
 * iteration: PMMG_create_oldGrp (src/grpsplit_pmmg.c:207-418) copies the
 * adjacency computed by MMG3D_hashTetra (src/libparmmg1.c:495,730), rebuilds
 * the boundary trias (MMG5_chkBdryTria, :404) and hashes the tria adjacency
 * (MMG3D_hashTria, :410).  These two entry points build the same arrays on
 * the device from the connectivity, so the arrays pmmg_hip_set_background*
 * consumes never take a host round trip.  All pointers are device memory on
 * the context's device, 16-byte aligned; calls are synchronous. */

/* Tetra adjacency of a conforming mesh from tetv[4*ne] (1-based vertex ids):
 *   adja[4*ne]  (may be NULL)  4*k'+i' of the tetra sharing face i, 0 on the boundary
 *   tet8[8*ne]  (may be NULL)  packed {v[4], adja[4]} records (set_background_tet8)
 * Returns 0 (message in pmmg_hip_last_error) for ids outside [1, np], repeated
 * ids in a tetra, or a face shared by more than two tetra. */
int pmmg_hip_build_adjacency(pmmg_hip_ctx *ctx, int np, int ne, const int *tetv,
                             int *adja, int *tet8);

/* Boundary trias: the faces with no neighbour — and, when tref[ne] (the
 * tetra references, MMG5_Tetra.ref) is given, the faces towards a neighbour
 * of smaller reference (MMG5_chkBdryTria's rule for a multi-material old mesh,
 * restated from Mmg @889d408: unpinned) — in (tetra, face) order, with
 * vertices v[MMG5_idir[i]] (outward for positively oriented tetra), and their
 * adjacency adjt[3*nt] (3*t'+j' across edge j, 0 on borders and on edges of
 * more than two trias).  Tetra from tet8 (packed records) when non-NULL, else
 * from tetv + adja.  *nt receives the number of trias; when it exceeds `cap`
 * nothing is written and 0 is returned.  tref and adjt may be NULL. */
int pmmg_hip_build_boundary(pmmg_hip_ctx *ctx, int np, int ne, const int *tet8,
                            const int *tetv, const int *adja, const int *tref,
                            int cap, int *nt, int *triv, int *adjt);

/* Element quality in the interpolated metric:
 * replaces MMG3D_tetraQual(mesh, met, 1) inside PMMG_tetraQual
 * (src/quality_pmmg.c:720-733, called at src/libparmmg1.c:845).  Device
 * pointers (the metric where pmmg_hip_locate_interp wrote it), synchronous:
 *   qual[ne]   pt->qual of every tetra (Mmg's unscaled caltet value; 0 for
 *              unused tetra, tetv row with v[0] <= 0)
 *   *minqual   MMG3D_ALPHAD * min over used tetra (2 when none is used)
 * met_size 0/1: geometric quality (MMG5_caltet_iso); 6: MMG5_caltet_ani with
 * the metric averaged over the 4 vertices.  As in the reference, a caller
 * treats *minqual == 0 as the "Quality computation problem" failure.
 * Returns 1, or 0 on invalid arguments. */
int pmmg_hip_tetra_qual(pmmg_hip_ctx *ctx, int np, const double *xyz, int ne,
                        const int *tetv, int met_size, const double *met,
                        double *qual, double *minqual);

/* ---- Reports on the adapted mesh in its interpolated metric -------------------
 * The two reports ParMmg prints after an adaptation, reduced on the device
 * from arrays that are already there (the metric where pmmg_hip_locate_interp
 * wrote it, qual where pmmg_hip_tetra_qual wrote it).  Device pointers,
 * 1-based vertex ids, synchronous, main stream only; return 1, or 0 with
 * pmmg_hip_last_error.  Both structs end in a zeroed reserved[4]; a shim
 * checks pmmg_hip_qual_histo_size() / pmmg_hip_len_histo_size() against its
 * sizeof at load, as it checks pmmg_hip_stats_size(). */

/* Quality histogram of one group: the per-group MMG3D_computeOutqua call of
 * PMMG_qualhisto (src/quality_pmmg.c:156-345, called at src/libparmmg1.c:910);
 * the MPI reductions of :275-304 stay on the host.  Restated from Mmg
 * @889d408, which is not in the image: parity unpinned.  With
 * rap = MMG3D_ALPHAD * qual[k] over the used tetra (tetv[4k] > 0): */
typedef struct {
  int64_t ne_used;     /* used tetra */
  double max;          /* largest rap (start value 0) */
  double min;          /* smallest rap (start value 2: none used, as pmmg_hip_tetra_qual) */
  int64_t iel;         /* 1-based row of the lowest-index used tetra attaining min, 0 when none; Mmg's
                          ordinal for a packed mesh (MMG5_paktet, src/libparmmg1.c:769) */
  double avg_sum;      /* sum of rap: the caller divides (src/quality_pmmg.c:322, after its MPI_Reduce) */
  int64_t good;        /* rap > 0.12 */
  int64_t med;         /* rap > 0.5 */
  int64_t his[5];      /* bin min(4, (int)(5 rap)) */
  int64_t reserved[4]; /* zero.  Mmg's ridge-point count nrid needs its point tags: not modelled */
} pmmg_hip_qual_histo_t;
int64_t pmmg_hip_qual_histo_size(void);

/* qual[ne] as pmmg_hip_tetra_qual wrote it, tetv[4*ne] 16-byte aligned.
 * Two calls on the same inputs fill byte-identical structs (avg_sum is summed
 * in a fixed order). */
int pmmg_hip_qual_histo(pmmg_hip_ctx *ctx, int ne, const int *tetv, const double *qual,
                        pmmg_hip_qual_histo_t *out);

/* Edge lengths in the metric: the body of PMMG_computePrilen
 * (src/quality_pmmg.c:370-574; PMMG_prilen :591-715 prints it), over every
 * unique edge {a, b} of the used tetra.  The owner of an edge is the
 * lowest-index used tetra holding it and, in that tetra, its lowest local
 * edge ia in MMG5_iare order: what MMG5_hashPop leaves in the ascending loop
 * of :506-564.  Its length is taken there, from (np, nq) = (v[iare[ia][0]],
 * v[iare[ia][1]]), with MMG5_lenedg (met_size 1: MMG5_lenedgCoor_iso, 6:
 * MMG5_lenedgCoor_ani, restated from Mmg @889d408: parity unpinned; any other
 * met_size returns 0).  Not modelled, as in pmmg_hip_compute_wgt_*: Mmg's
 * metric storage at ridge points and the MG_GEO point filter of :510-517. */
typedef struct {
  int64_t nedge;       /* unique edges, skipped ones included */
  int64_t nskipped;    /* mesh edges found in the skip list: counted here and nowhere else */
  int64_t ned;         /* analysed edges with len != 0 */
  int64_t nnull;       /* analysed edges with len == 0 */
  double avlen_sum;    /* sum of len over the ned edges, in a fixed order (the caller divides) */
  double lmin;         /* shortest of them (start value 1e30), strict <: ties go to the earlier (owner, ia) */
  double lmax;         /* longest (start value 0), strict > */
  int32_t amin, bmin;  /* (np, nq) of the shortest edge at its owner, 0 when there is none */
  int32_t amax, bmax;  /* of the longest */
  int64_t hl[9];       /* hl[i] for the first i < 8 with bd[i] <= len && len < bd[i+1], else hl[8], bd = 0,
                          0.3, 0.6, 0.7071, 0.9, 1.3, 1.4142, 2, 5 (:489-495: a NaN length lands in
                          hl[8] and moves neither extreme) */
  int64_t reserved[4]; /* zero */
} pmmg_hip_len_histo_t;
int64_t pmmg_hip_len_histo_size(void);

/*   skip[2*nskip]     (NULL with nskip 0) vertex-id pairs, any orientation, repeats allowed: the parallel
 *                     edges a lower rank owns (:412-452).  A pair that is no mesh edge is ignored.
 *   edge_out[2*cap], len_out[cap]   (either may be NULL) the analysed edges (skipped ones left out, null
 *                     ones included) as (np, nq) and their lengths, in ascending (owner tetra, ia)
 *                     order.  When cap < nedge - nskipped nothing is written to them, *out is still
 *                     filled and 0 is returned (pmmg_hip_build_boundary's convention).
 * A vertex id of a used tetra outside [1, np] returns 0.  tetv 16-byte, skip / edge_out / len_out 8-byte
 * aligned; needs 6 ne < 2^32.  The edge table lives in the context (pmmg_hip_release_scratch).
 * Two calls on the same inputs give byte-identical out, edge_out and len_out. */
int pmmg_hip_edge_lengths(pmmg_hip_ctx *ctx, int np, const double *xyz, int ne, const int *tetv,
                          int met_size, const double *met, int nskip, const int *skip,
                          pmmg_hip_len_histo_t *out, int cap, int *edge_out, double *len_out);

/* Device bytes of the two reports' scratch held by the context (edge table, slabs; 0 after
 * pmmg_hip_release_scratch). */
int64_t pmmg_hip_mesh_stats_bytes(pmmg_hip_ctx *ctx);

/* Solutions as packed per-vertex records: rec[RS*np], vertex v's record at
 * rec + RS*(v-1) = [metric (met_size) | field 0 | field 1 | ...] with
 * RS = (met_size + sum field_size) rounded up to even.  The module's
 * preferred HBM layout (one 128-byte line per vertex for up to 16 doubles:
 * one gather per vertex instead of one per solution); a shim builds it in the
 * pass that packs MMG5_Point.c.  Supported: at most 16 doubles in the
 * compiled slot layouts (BASELINE's configs: metric, scalar, vector, tensor;
 * iso metric + scalars); otherwise 0 is returned and pmmg_hip_set_solutions
 * takes the arrays.  Device records: 16-byte aligned (RS * 8 bytes apart: a
 * 128-byte-aligned base puts a 16-double record on one cache line).
 * Returns 1/0. */
int pmmg_hip_set_solutions_packed(pmmg_hip_ctx *ctx, int met_size, int nfield,
                                  const int *field_size, const double *rec, int where);

/* pmmg_hip_locate_interp with the new points' values written as records of
 * the same layout as the packed input (rec_out[RS*np_new], point ip's record
 * at rec_out + RS*(ip-1): [metric | field 0 | ...]): after
 * pmmg_hip_set_solutions_packed, device pointers only (rec_out 16-byte
 * aligned; 128-byte aligned puts each 16-double record on one line).  What a
 * record is not written for keeps its previous content, per solution as in
 * the reference (skipped points, MMG5_invmat failures).  The records a step
 * writes are the next iteration's background records as they are (the
 * adapted group becomes the old group, src/libparmmg1.c:653): a resident
 * pipeline never repacks.  Same results, bit for bit, as
 * pmmg_hip_locate_interp.  Returns 1/0. */
int pmmg_hip_locate_interp_rec(pmmg_hip_ctx *ctx, int np_new, const double *xyz_new, const uint8_t *pclass,
                               double *rec_out, int *elem_out, int8_t *hit_out, pmmg_hip_stats *stats, int where);

/* Load-balancing weights from the interpolated metric (SURVEY.md §8(f)
 * rank 2, the second consumer after PMMG_tetraQual), device arrays, 1-based
 * vertex ids, synchronous.
 *
 * pmmg_hip_compute_wgt_mesh replaces PMMG_computeWgt_mesh
 * (src/metis_pmmg.c:242-266): for every used tetra k (tetv[4k] > 0) with an
 * xtetra (xt[k] != 0), qual[k] = sum over its faces f with (ftag[4k+f] & tag)
 * of PMMG_computeWgt(mesh, met, pt, f) (:280-300); the other entries of qual
 * are left untouched.  ftag = the xtetra face tags gathered per tetra
 * (pxt->ftag[0..3]).
 *
 * pmmg_hip_compute_wgt_faces: PMMG_computeWgt of a list of faces
 * face[2j] = tetra (1-based), face[2j+1] = local face index (the graph
 * weights of src/metis_pmmg.c:812, :959) into wgt[j].
 *
 * PMMG_computeWgt: the three edges of the face have lengths len in the
 * metric (MMG5_lenedg: met_size 1 MMG5_lenedgCoor_iso, 6
 * MMG5_lenedgCoor_ani); res = sum (len - 1) for len <= 1 else (1/len - 1);
 * weight = min(1/exp(28 res / 3), PMMG_WGTVAL_HUGEINT); met_size 0 (no
 * metric): PMMG_WGTVAL_HUGEINT.  Mmg's special metric storage at ridge
 * points (MG_GEO edges of an aniso metric) is not modelled.
 * Returns 1, or 0 on invalid arguments. */
int pmmg_hip_compute_wgt_mesh(pmmg_hip_ctx *ctx, int np, const double *xyz, int ne,
                              const int *tetv, const int *xt, const uint16_t *ftag,
                              int met_size, const double *met, int tag, double *qual);
int pmmg_hip_compute_wgt_faces(pmmg_hip_ctx *ctx, int np, const double *xyz,
                               const int *tetv, int nface, const int *face,
                               int met_size, const double *met, double *wgt);

/* ---- The METIS element graph of a group (src/metis_pmmg.c:746-823) ----------
 * PMMG_graph_meshElts2metis on the device: the CSR dual graph of a group's
 * tetra that PMMG_part_meshElts2metis (:1293) hands to METIS at the group
 * split (src/grpsplit_pmmg.c:1698) and the distribution
 * (src/distributemesh_pmmg.c:1026, :1139), from the adapted mesh and the
 * metric where pmmg_hip_locate_interp wrote it.  Device pointers, 1-based
 * vertex ids, synchronous, main stream only.
 *   tetra   from tet8 (packed {v[4], adja[4]} records) when non-NULL, else
 *           from tetv + adja; with tet8 == NULL && adja == NULL the adjacency
 *           is built first (pmmg_hip_build_adjacency's kernels, into context
 *           scratch): MMG3D_hashTetra's branch of :756, with that function's
 *           failures and messages.  tetv may be NULL when adja is given and
 *           adjwgt is NULL (every row then counts as used).
 *   xadj[ne+1]      xadj[0] = 0, xadj[k] = non-zero adja entries of rows 0..k-1
 *   adjncy[cap]     adja / 4 - 1 of every non-zero entry in ascending
 *                   (tetra, face) order: the loop of :801-818
 *   *nadjncy        (host) the entry count xadj[ne].  The reference's
 *                   ++(*nadjncy) of :783 is slack for its allocation and is
 *                   not reproduced.
 *   adjwgt[cap]     (may be NULL: the unweighted graph of the distribution and
 *                   of the last iteration, :790; xyz and met are then not
 *                   touched and may be NULL)  max((int)w, 1) with w =
 *                   PMMG_computeWgt of the face: for met_size 1 / 6 the bits
 *                   pmmg_hip_compute_wgt_faces gives for that (tetra, face);
 *                   met_size 0 (no metric): PMMG_WGTVAL_HUGEINT; a w that is
 *                   not finite gives 1.  Mmg's metric storage at ridge points
 *                   is not modelled (as in pmmg_hip_compute_wgt_*).
 * An unused tetra (tetv row with v[0] <= 0) gets an empty row whatever its
 * adja row holds.  Returns 0 (message in pmmg_hip_last_error), with nothing
 * written to adjncy / adjwgt, when
 *   - cap < *nadjncy: xadj and *nadjncy are still filled
 *     (pmmg_hip_build_boundary's convention: call with cap 0 to size);
 *   - an adja entry lies outside [4, 4*ne+3], or points to an unused tetra
 *     (the reference requires a packed mesh);
 *   - weights are asked and a used tetra has a vertex id outside [1, np];
 *   - ne >= 2^29 (the 4*k+i encoding, as pmmg_hip_set_background).
 * tet8 / tetv / adja / xyz / met 16-byte, xadj / adjncy / adjwgt 4-byte
 * aligned.  idx_t is 32 bits (METIS 5.1.0's default IDXTYPEWIDTH); there is no
 * 64-bit variant.  Per-block counts and a built adjacency live in the context
 * (pmmg_hip_release_scratch).  Two calls on the same inputs give
 * byte-identical outputs. */
int pmmg_hip_metis_graph(pmmg_hip_ctx *ctx, int np, const double *xyz, int ne,
                         const int *tetv, const int *adja, const int *tet8,
                         int met_size, const double *met,
                         int cap, int64_t *nadjncy,
                         int *xadj, int *adjncy, int *adjwgt);

/* ---- Contiguity of a partition: the subgroups of a part, and their fix ------
 * What the reference does with the same two inputs as the graph, the tetra
 * adjacency and a colour per tetra, right after METIS:
 * PMMG_check_part_contiguity (src/metis_pmmg.c:312), PMMG_check_grps_contiguity
 * (:446, one colour: part == NULL) and PMMG_check_contiguity
 * (src/moveinterfaces_pmmg.c:309) count the subgroups of every colour;
 * PMMG_fix_contiguity (:475-523, through PMMG_fix_contiguity_centralized :577
 * and PMMG_fix_contiguity_split :534) merges all but the largest subgroup of
 * every colour into a neighbouring colour.  A subgroup is a connected
 * component of the adjacency graph restricted to one colour.  Device pointers
 * unless marked host, synchronous, main stream only.
 *   tetra   from tet8 when non-NULL, else from adja; tetv may be NULL (every
 *           row then counts as used); with tet8 == NULL && adja == NULL the
 *           adjacency is built first from tetv (pmmg_hip_build_adjacency's
 *           kernels, into context scratch, with that function's failures and
 *           messages; np is taken as the largest vertex id).  A tetra with
 *           v[0] <= 0 is unused: it belongs to no subgroup, its part is never
 *           written and has no influence on any output.  The adjacency must be symmetric, as
 *           MMG3D_hashTetra's is; this is not checked.
 *   part[ne]        the colour of every tetra, in [0, ncolor); NULL: one
 *                   colour for the whole mesh (ncolor must be 1).
 * pmmg_hip_part_subgroups:
 *   head[ne]        (may be NULL) the lowest tetra of the subgroup, 1-based; 0
 *                   for an unused tetra
 *   flag[ne]        (may be NULL) 1 + the number of subgroups of the same
 *                   colour with a lower head: the value the reference's sweeps
 *                   leave in flag (src/metis_pmmg.c:347, :486); 0 for an
 *                   unused tetra
 *   ncomp[ncolor]   (host) subgroups per colour
 *   sub[cap], *nsub (host) the table in ascending head and its length;
 *                   cap < *nsub returns 0 with *nsub, ncomp, head and flag
 *                   filled and nothing written to sub (call with cap 0 to size)
 *   *rounds         (host, may be NULL) hooking rounds of the labelling, at
 *                   most 2 ceil(log2 ne) + 1 (2 for ne = 1)
 * pmmg_hip_fix_contiguity: PMMG_fix_contiguity for colours 0 .. ncolor-1 (the
 * centralized call's PMMG_set_color(igrp) == igrp).  For c ascending: the
 * subgroups of colour c in the current part, in ascending head; main = the
 * first; for every later one, next: if next.size > main.size, main takes the
 * colour across its exit and next becomes main (main.exit == 0: nothing moves,
 * main stays, *nstuck++); otherwise next takes the colour across its exit
 * (next.exit == 0: *nstuck++).  The colour's changes are applied before colour
 * c + 1 is looked at.  *nmerged counts the moved subgroups, *nmoved their
 * tetra.
 * Deviation: the reference moves a subgroup to the colour of the first foreign
 * neighbour in BFS order from its head (list_otetra, :280-296), a property of
 * a sequential traversal; this call takes the lowest (tetra, face) of the
 * subgroup whose neighbour has another colour, the table's `exit`.  The two
 * agree where a subgroup's head lies on its rim.
 * Returns 0 (message in pmmg_hip_last_error) with nothing written to part, sub,
 * head or flag when a link lies outside [4, 4*ne+3] or points to an unused
 * tetra, a used tetra's part lies outside [0, ncolor), part == NULL with
 * ncolor != 1, or ne >= 2^29.  tet8 / tetv / adja 16-byte, part / head / flag
 * 4-byte aligned.  Labels and the table live in the context
 * (pmmg_hip_release_scratch).  Two calls on the same inputs give
 * byte-identical outputs. */
typedef struct {
  int color;  /* the part the subgroup belongs to */
  int head;   /* its lowest tetra, 1-based: where the reference's scan opens its list */
  int size;   /* tetra in it */
  int exit;   /* 4*k+f (k 1-based) of the lowest (tetra, face) of the subgroup whose
                 neighbour has another colour; 0: it touches no other colour */
} pmmg_hip_subgroup;

int pmmg_hip_part_subgroups(pmmg_hip_ctx *ctx, int ne, const int *tetv, const int *adja,
                            const int *tet8, const int *part, int ncolor,
                            int *head, int *flag,
                            int *ncomp,
                            int cap, pmmg_hip_subgroup *sub, int64_t *nsub,
                            int *rounds);

int pmmg_hip_fix_contiguity(pmmg_hip_ctx *ctx, int ne, const int *tetv, const int *adja,
                            const int *tet8, int *part, int ncolor,
                            int64_t *nmoved, int *nmerged, int *nstuck);

/* Diagnostic, not part of the reference's interface: flatten passes of the
 * context's last contiguity call (reported by tools/contiguity_time.py); -1
 * without a context. */
int64_t pmmg_hip_contig_passes(pmmg_hip_ctx *ctx);

/* ---- Group split: the sub-meshes and interfaces of a partition -------------
 * What the reference does with the repaired part: PMMG_split_grps
 * (src/grpsplit_pmmg.c:1711) through PMMG_split_eachGrp (:1267-1445) and
 * PMMG_splitGrps_fillGroup (:819-1094) cuts, for every colour, a mesh of its
 * own out of the group.  The reference's loop is sequential; its result is a
 * function of (tetv, adja, part), stated here and computed on the device.
 * Device pointers unless marked host, synchronous, main stream only, 1-based
 * ids; tetra from tet8 when non-NULL, else from tetv + adja (both needed).
 *   Tetra.  The tetra of group g are the old tetra with part == g, in
 *     ascending old id.  old_tet[ne] holds the old id of every new tetra, the
 *     groups one after the other in colour order; new_tet[k] (may be NULL) is
 *     the 1-based rank of old tetra k in its group (the reference's pt->flag).
 *   Points.  Over the group's tetra in new order and the corners 0..3 of each,
 *     a vertex gets the group's next id the first time it appears (:879-999).
 *     A vertex used by several groups is a point of each.  tetv_out holds
 *     these ids, old_pt the old id of every new point, groups concatenated.
 *   Adjacency.  adja_out[new k][f] = 4*new_tet[j] + i where the old link 4j+i
 *     stays inside the group; 0 where the neighbour has another colour or the
 *     old entry was 0 (:1012-1076).  tet8_out packs {tetv_out, adja_out} rows.
 *     Each of tetv_out, adja_out, tet8_out may be NULL.
 *   Face list of group g (face2int_face_comm_index1 / _index2), in (new tetra
 *     t, face f) order, t 1-based: an entry for (a) an old boundary face with
 *     face_old >= 0: index1 = 12t + 3f + face_old % 3, index2 = face_old / 3;
 *     (b) a face whose neighbour has another colour.  The side with the lower
 *     colour owns the face; the owned faces are numbered nface0, nface0+1, ...
 *     in (colour, new tetra, face) order over the whole call, and index2 is
 *     that number on both sides.  On the owner's side iploc = 0; on the other
 *     side iploc is the position, in MMG5_idir[f], of the owner's vertex
 *     v[MMG5_idir[i][0]] (i the owner's face; :692-743).  index1 = 12t + 3f +
 *     iploc.  *nface_end = nface0 + the number of owned faces.
 *   Node list of group g (node2int_node_comm_index1 / _index2).  One counter
 *     runs over the call: E, the entries appended so far, starting at nnode0.
 *     The reference's int_node_comm->nitem counts appended entries, not
 *     distinct nodes (:630 and :664 both increment it), so the positions have
 *     gaps; this is reproduced.  A group appends two runs.  First, in
 *     ascending new point id, every point of g that already has a position
 *     (from node_pos, or given by a lower colour): index1 = the new id,
 *     index2 = the position.  Then the group's new interface nodes: points
 *     without a position on a face of g towards another colour, in order of
 *     their first (new tetra, face, MMG5_idir[f][0..2]) occurrence (:606-637,
 *     :1081-1091); the j-th (0-based) gets index2 = E' + j + 1, E' being E
 *     after the first run.  *nnode_end is the final E.  A node's owner is the
 *     lowest colour that has it on an interface face.
 *   count[ngrp] (host) the tetra, points, face entries and node entries of
 *     every group; group g's segments of the outputs start at the exclusive
 *     prefix sums of count[].ne, .np, .nface, .nnode.
 * Out of scope: xtetra / xpoint records; the MG_PARBDY / MG_PARBDYBDY tags
 * (the two lists name exactly the faces and points that get them); ls / disp
 * (gather them with pmmg_hip_gather_rows); reallocation and cleanMesh; the
 * external (MPI) communicators.
 * Returns 0 (message in pmmg_hip_last_error) with nothing written to any
 * device output when a part value lies outside [0, ngrp), a tetra is unused
 * (v[0] <= 0: the reference requires a packed mesh, :1461), a link lies
 * outside [4, 4*ne+3], a vertex id lies outside [1, np], or ne >= 2^29.
 * Returns 0 as well when a cap is smaller than its total: count, *nnode_end
 * and *nface_end are still filled, old_tet / new_tet / tetv_out / adja_out /
 * tet8_out may be written, and none of old_pt or the four lists is (call with
 * caps of 0 to size: pmmg_hip_build_boundary's convention).  ne == 0 and empty
 * colours are valid; their counts are 0.  tet8 / tetv / adja / tetv_out /
 * adja_out / tet8_out 16-byte, every other array 4-byte aligned.  Scratch
 * lives in the context (pmmg_hip_release_scratch).  Two calls on the same
 * inputs give byte-identical outputs. */
typedef struct { int ne, np, nface, nnode; } pmmg_hip_split_count;

int pmmg_hip_split_groups(pmmg_hip_ctx *ctx, int np, int ne,
        const int *tetv, const int *adja, const int *tet8,
        const int *part, int ngrp,
        const int *node_pos,   /* [np]   may be NULL: old node2int_node_comm_index2 of the point, -1 none   */
        const int *face_old,   /* [4*ne] may be NULL: 3*pos + iploc of an old parallel face, -1 none        */
        int nnode0, int nface0,/* int_node_comm->nitem / int_face_comm->nitem on entry                      */
        pmmg_hip_split_count *count,            /* host [ngrp]: always filled on a valid input             */
        int64_t pt_cap, int64_t face_cap, int64_t node_cap,
        int *old_tet,          /* [ne]  old id of every new tetra, groups concatenated in colour order      */
        int *new_tet,          /* [ne]  may be NULL: id of every old tetra inside its group (pt->flag)      */
        int *tetv_out, int *adja_out, int *tet8_out,   /* [4ne],[4ne],[8ne]; each may be NULL               */
        int *old_pt,           /* [pt_cap] old id of every new point, groups concatenated                   */
        int *face_idx1, int *face_idx2,         /* [face_cap] face2int_face_comm_index1 / _index2           */
        int *node_idx1, int *node_idx2,         /* [node_cap] node2int_node_comm_index1 / _index2           */
        int *nnode_end, int *nface_end);        /* host: the two nitem on exit                              */

/* out row r = in row src[r]-1, r < n, rows of `size` doubles: the point rows
 * (xyz: 3), the metric and the fields of a group through its old_pt.  src
 * 4-byte, in / out 8-byte aligned; every src[r] must name a row of `in` (not
 * checked).  Synchronous. */
int pmmg_hip_gather_rows(pmmg_hip_ctx *ctx, int64_t n, const int *src /*1-based*/, int size,
                         const double *in, double *out);

/* Diagnostic: first-use rounds of the context's last split (the most colours
 * that met at one vertex; tools/split_groups_time.py); -1 without a context. */
int pmmg_hip_split_rounds(pmmg_hip_ctx *ctx);

/* ---- Group merge: the groups of a rank joined into one mesh ----------------
 * The inverse of the split, and the first statement of PMMG_split_n2mGrps
 * before every redistribution: PMMG_merge_grps steps 0-4
 * (src/mergemesh_pmmg.c:1004-1043; PMMG_mergeGrps_interfacePoints :433-469
 * with _addGrpJ :303-422, PMMG_mergeGrpJinI_internalPoints :480-571,
 * _interfaceTetra :584-682, _internalTetra :695-751, PMMG_set_color_tetra,
 * src/moveinterfaces_pmmg.c:119-134).  The reference's loop is sequential; what
 * it leaves in group 0 and in the two intvalues arrays is a function of its
 * inputs, stated here and computed on the device.  Device pointers unless
 * marked host, synchronous, main stream only, 1-based ids.
 *   Input.  The groups concatenated in group order, as pmmg_hip_split_groups
 *     writes them: count[g] = {ne, np, nface, nnode}, tetra rows with ids local
 *     to their group (tet8 records when non-NULL, else tetv; links not read),
 *     the node and face lists.  e is an entry's index in the concatenated node
 *     (or face) list: ascending e is ascending (group, entry).  nnode / nface
 *     are int_node_comm->nitem / int_face_comm->nitem.
 *   Points.  A point of group 0 keeps its id.  For a group g >= 1, a point's
 *     entry is the first entry of g's node list that names it (later ones are
 *     skipped, :346) and its position that entry's index2.  Every entry of
 *     group 0 holds its position (:452-459).  A listed point of g >= 1 whose
 *     position group 0 holds takes group 0's id there (its index1).  The
 *     other listed positions each become one new point, numbered np_0 + 1,
 *     np_0 + 2, ... in ascending e of the position's lowest entry (step 1,
 *     over all groups); every point listed at the position takes that id.
 *     Then, group by group for g = 1, 2, ..., the points of g that no entry
 *     names are numbered in ascending id (step 2).  new_pt[i] is the merged id
 *     of concatenated point i (pptJ->tmp), src_pt[q - 1] the 1-based row, in the
 *     concatenated points, of the point that made merged point q: its own row
 *     for group 0, the lowest entry's point for a created one.
 *   node_val[p] is int_node_comm->intvalues[p] after step 4: 0 where nobody
 *     holds p; else the merged id of the point at p, negated once for every
 *     further group that holds p (:400-401): the sign is (-1)^(holders - 1).
 *   Tetra.  Group 0's tetra keep their ids; group g's get the ids from
 *     ne_0 + ... + ne_(g-1) + 1 on: first g's interface tetra (those named by
 *     an entry of g's face list, iel = index1 / 12) in order of their first
 *     entry, then g's other tetra in ascending id.  tetv_out holds the
 *     vertices renamed through new_pt, corner order kept; new_tet[k] the
 *     merged id of concatenated tetra k (ptJ->flag), src_tet[m - 1] the 1-based
 *     concatenated row of merged tetra m.  mark_out[m - 1] = color[g] of the
 *     tetra's group (PMMG_GRPSPL_DISTR_TARGET).
 *   face_val[q] is int_face_comm->intvalues[q] after step 4: 0 where no entry
 *     names q; else the value of q's lowest entry, index1 as it stands for an
 *     entry of group 0 (:1008-1014) and 12 * merged tetra + index1 % 12 for a
 *     group g >= 1, negated by every later entry of a group g >= 1 with that
 *     position (:629-631, :657-658).
 * Preconditions, the reference's own: every group packed (no unused tetra or
 * point, group 0's free lists in order); within one group a node position
 * names one point and a face position appears once.  The last two are not
 * checked: the outputs then still are ids in range.  With one group the
 * reference returns before it allocates the intvalues (:990); the statement
 * above is applied all the same.
 * Out of scope, gathered by the caller through src_pt / src_tet
 * (pmmg_hip_gather_rows, pmmg_hip_gather_rows_i32): xtetra / xpoint records,
 * ref, qual, tags, the solution rows; reallocation;
 * PMMG_mergeGrps_communicators and PMMG_updateTag, which take node_val /
 * face_val as the two intvalues; the adjacency, which the reference frees
 * (:987): pmmg_hip_build_adjacency on tetv_out rebuilds it.
 * Returns 0 (message in pmmg_hip_last_error) with nothing written to any
 * device output when a vertex id lies outside [1, np_g], a node index1
 * outside [1, np_g], a node index2 outside [0, nnode), a face index1 / 12
 * outside [1, ne_g], a face index2 outside [0, nface), the tetra of all
 * groups reach 178956970 (12 * ie + 11 must fit an int, the reference's limit
 * too), the points, the entries of a list or the positions reach 2^29, or an
 * array is misaligned (tetv / tet8 / tetv_out 16 bytes, every other 4).
 * Returns 0 as well when pt_cap is smaller than the merged points: *np_out and
 * *ne_out are filled and no device output is written (call with pt_cap = 0 to
 * size).  ngrp == 1, empty groups and no tetra at all are valid.  Scratch
 * lives in the context (pmmg_hip_release_scratch).  Two calls on the same
 * inputs give byte-identical outputs. */
int pmmg_hip_merge_groups(pmmg_hip_ctx *ctx, int ngrp, const pmmg_hip_split_count *count /*host*/,
        const int *tetv, const int *tet8,            /* [sum ne] rows, group-local ids; tet8 wins, links not read */
        const int *node_idx1, const int *node_idx2,  /* [sum nnode] */
        const int *face_idx1, const int *face_idx2,  /* [sum nface] */
        int nnode, int nface,                        /* the two int_*_comm->nitem */
        const int *color,                            /* host [ngrp] or NULL (then mark_out must be NULL) */
        int64_t pt_cap,
        int *new_pt,   /* [sum np] merged id of every input point (pptJ->tmp)            */
        int *new_tet,  /* [sum ne] merged id of every input tetra (ptJ->flag), may be NULL */
        int *src_pt,   /* [pt_cap] 1-based row in the concatenated points of every merged point */
        int *src_tet,  /* [sum ne] 1-based row in the concatenated tetra of every merged tetra  */
        int *tetv_out, int *mark_out,                /* [4 sum ne], [sum ne]; each may be NULL */
        int *node_val, int *face_val,                /* [nnode], [nface]; each may be NULL */
        int *np_out, int *ne_out);                   /* host */

/* pmmg_hip_gather_rows for rows of `size` ints: the ref / mark rows of the
 * merged tetra through src_tet.  src, in, out 4-byte aligned; every src[r] must
 * name a row of `in` (not checked).  Synchronous. */
int pmmg_hip_gather_rows_i32(pmmg_hip_ctx *ctx, int64_t n, const int *src /*1-based*/, int size,
                             const int *in, int *out);

/* ---- Interface displacement: move the group fronts by layers ----------------
 * PMMG_mark_interfacePoints and the layer loop of PMMG_part_moveInterfaces
 * (src/moveinterfaces_pmmg.c:1052-1090, :1366-1439; PMMG_REDISTRIBUTION_
 * ifc_displacement, called from PMMG_split_n2mGrps before every group
 * redistribution), as a function of their inputs: the old groups' interfaces
 * advance by layers of vertex stars into the group of larger weight.  Followed
 * by pmmg_hip_fix_contiguity (:1446) the marks are the `part` that
 * pmmg_hip_split_groups consumes.  PMMG_check_reachability and the MPI
 * exchange between two layers stay with the shim.
 *
 * Colours are indices in [0, ncolor) (the shim maps its nprocs*igrp+rank ids);
 * weight[c] > 0 is the priority map's entry (mapgrp: the group's tetra
 * count); "c beats d" means weight[c] < weight[d], strictly
 * (PMMG_get_ifcDirection(d, c) == 1).  A used tetra has v[0] > 0; an unused
 * one never changes and never influences anything.  Ids are 1-based; point p
 * is entry p-1 of ptcolor / ptfront.
 *
 * Seed.  ptcolor[p] is the mark at the lowest corner 4*ie+iloc of p whose
 * weight is the minimum over p's corners; p is front iff the mark at p's
 * lowest corner does not have that minimum weight (the reference flags a
 * point only when its colour changes after its first corner: an interface
 * point whose first tetra already holds the winning colour is not front).  A
 * point of no used tetra gets colour -1 and is not front.
 *
 * One layer.  The front points' colours do not change during a layer.
 *  1. Each used tetra T takes its front points in ascending id and keeps a
 *     running strict minimum of weight that starts at its own mark.  Every
 *     point whose colour beats the running colour is an event (T, ip, C =
 *     ptcolor[ip], previous colour).  T's new mark is the last event's colour;
 *     between equal weights the lower ip wins.
 *  2. A point q off the front in a tetra with an event is front for the next
 *     layer.  It takes the colour of the event of least (weight[C], ip) over
 *     all events of the tetra that contain q, if that colour beats ptcolor[q].
 *  3. A front point other than ip in a tetra with an event is a side point: it
 *     takes the new mark of the tetra of least (weight, tetra id) among all
 *     tetra that contain it, if that beats its own colour, and is front for
 *     the next layer.
 *  4. Every other front point leaves the front.
 *  5. Before every layer the points of set_pt (a shim's communicator points)
 *     become front; before the first layer of a call they take set_color[i]
 *     when it is given.  The entries of set_pt are distinct.
 *
 * The brake.  Every event whose previous colour g is local (nelem[g] >= 0;
 * -1: not local) takes one off nelem[g], the events between the first and the
 * last of a tetra included, whose colour never gained the tetra.  The
 * reference stops in the middle of a ball when a count reaches nemin[g] =
 * MG_MIN(PMMG_REDISTR_NELEM_MIN = 6, negrp0/2 + 1); what it leaves then
 * depends on its traversal order and is not computed here.  With D[g] the
 * layer's events by previous colour, no brake fires in the layer iff D[g] <=
 * nelem[g] - nemin[g] for every local g with D[g] > 0.  A layer is computed
 * into scratch and committed only if that holds; otherwise nothing of that
 * layer is committed, *blocked = 1, *layers_done counts the layers before it
 * and every output holds their result, without the set points of the layer
 * that was dropped: the state the reference is in before that layer, from
 * which a shim finishes with the reference's own loop.
 *
 * Two deliberate deviations (pinned by tests/
 * test_moveifc_ref_host.py).  Side points: between two different colours of
 * equal least weight the reference takes the first tetra in its BFS order, the
 * module the lowest tetra id.  Ball and star: the reference's ball is the
 * face-connected part of the vertex star around the point's handle s, the
 * module's is the whole star; s is not an output, and the MMG3D_LMAX overflow
 * failure has no counterpart.
 *
 * Pointers are device pointers unless marked host.  Synchronous, main stream
 * only.  tet8 wins over tetv; either gives the vertices (the links are not
 * read).  Returns 0 with a message and nothing written: a mark of a used tetra
 * or a colour outside [0, ncolor), weight[c] <= 0, a vertex id outside [1, np],
 * a set_pt entry outside [1, np], ne >= 2^29, tet8 / tetv not 16-byte or
 * another device array not 4-byte aligned (ptfront: any).  Scratch lives in a
 * cache of its own in the context (pmmg_hip_release_scratch).  Two calls on
 * the same inputs give byte-identical outputs. */
int pmmg_hip_ifc_seed(pmmg_hip_ctx *ctx, int np, int ne, const int *tetv, const int *tet8,
        const int *mark,              /* [ne]                                                  */
        int ncolor, const int *weight,/* host [ncolor]                                         */
        int *ptcolor,                 /* [np] out                                              */
        unsigned char *ptfront);      /* [np] out: 1 front, 0 not                              */

int pmmg_hip_ifc_layers(pmmg_hip_ctx *ctx, int np, int ne, const int *tetv, const int *tet8,
        int *mark,                    /* [ne] in / out                                         */
        int ncolor, const int *weight,/* host [ncolor]                                         */
        int *nelem,                   /* host [ncolor] in / out: negrp; -1 = not local         */
        const int *nemin,             /* host [ncolor]                                         */
        int *ptcolor, unsigned char *ptfront,   /* [np] in / out                               */
        int nset, const int *set_pt, const int *set_color,  /* [nset]; set_color may be NULL   */
        int nlayers,
        int *layers_done, int *blocked,         /* host                                        */
        int *moved);                  /* host [nlayers]: tetra re-marked per layer             */

/* The DISTR branch of PMMG_part_getInterfaces (:1176-1211): part[k] = the rank
 * of mark[k] among the colours present in a used tetra, counted in ascending
 * order[colour] (host [ncolor]: the colour's place in the caller's packing
 * order, the reference's (i + myrank) % nprocs loop); *ngrp (host) = the
 * colours present.  part of an unused tetra is 0.  The MMG branch is the
 * identity on indices and needs no call.  mark and part may be one array. */
int pmmg_hip_remap_colors(pmmg_hip_ctx *ctx, int ne, const int *tetv, const int *tet8, const int *mark,
                          int ncolor, const int *order, int *part, int *ngrp);

/* ---- One group split over the GPUs of a node -------------
 * One process per GPU (ParMmg's MPI ranks; GPU = node-local rank,
 * src/parmmg.c:121).  Each rank transfers its part of the group's new points
 * (its own pmmg_hip_locate_interp, against a replicated or halo-sharded
 * background), then the located element ids, hit codes and interpolated rows
 * of every part are collected on every rank with one RCCL all-gather over
 * xGMI.  ParMmg's only process boundary is MPI (src/libparmmg1.c:831); a shim
 * creates the communicator with MPI:
 *     char id[PMMG_HIP_COMM_ID_BYTES];
 *     if (rank == 0) pmmg_hip_comm_unique_id(id);
 *     MPI_Bcast(id, PMMG_HIP_COMM_ID_BYTES, MPI_BYTE, 0, comm_node);
 *     pmmg_hip_comm_init(ctx, nranks, rank, id);       (collective)
 * or hands over an ncclComm_t it owns (pmmg_hip_comm_attach).  RCCL
 * (librccl.so.1) is loaded at the first of these calls.  Returns 1/0. */
#define PMMG_HIP_COMM_ID_BYTES 128
int pmmg_hip_comm_unique_id(void *id);
int pmmg_hip_comm_init(pmmg_hip_ctx *ctx, int nranks, int rank, const void *id);
int pmmg_hip_comm_attach(pmmg_hip_ctx *ctx, void *nccl_comm, int nranks, int rank);

/* All-gather of the parts' results (collective over the communicator; every
 * rank passes the same counts[], nslot, slot_size[] and the same choice of
 * elem / hit given or NULL — the ranks first agree on that and on their
 * arguments' validity, and all return 0 together when one differs or fails):
 * counts[nranks] points per rank (rank order), this rank's part in
 * rows[s] (slot_size[s] doubles per point: the metric / field rows
 * pmmg_hip_locate_interp wrote), elem, hit (both optional, NULL on every
 * rank or on none); outputs rows_all[s], elem_all, hit_all hold the parts
 * concatenated in rank order (sum counts points).  Device pointers;
 * returns when the outputs are written.  Returns 1/0. */
int pmmg_hip_allgather_points(pmmg_hip_ctx *ctx, const int64_t *counts, int nslot, const int *slot_size,
                              const double *const *rows, double *const *rows_all, const int *elem, int *elem_all,
                              const int8_t *hit, int8_t *hit_all);

/* Device memory helpers for callers that keep data resident (bench, shims
 * that reuse buffers across iterations). */
void *pmmg_hip_malloc(pmmg_hip_ctx *ctx, int64_t bytes);
int   pmmg_hip_free(pmmg_hip_ctx *ctx, void *dptr);
int   pmmg_hip_memcpy_h2d(pmmg_hip_ctx *ctx, void *dst, const void *src, int64_t bytes);
int   pmmg_hip_memcpy_d2h(pmmg_hip_ctx *ctx, void *dst, const void *src, int64_t bytes);

/* Last error message of the context (static storage inside ctx). */
const char *pmmg_hip_last_error(pmmg_hip_ctx *ctx);

/* Number of visible HIP devices (0 when none / no driver). */
int pmmg_hip_device_count(void);

#ifdef __cplusplus
}
#endif

#endif /* PARMMG_HIP_H */
