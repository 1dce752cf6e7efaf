/*
 * pmmg_host.c — C host layer of the transfer step (see pmmg_host.h).
 * Product code: it calls only the HIP module's C-ABI; there is no CPU
 * fallback — a missing device makes every entry point return 0.
 */
#define _GNU_SOURCE
#include "pmmg_host.h"
#include "pmmg_stage.h"
#include <pthread.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <unistd.h>

/* ---------------------------------------------------------------- point classification
 * The visitation loop of src/interpmesh_pmmg.c:535-550 classifies every
 * vertex of a valid new tetra once: skipped if !MG_VOK or MG_REQ (copied by
 * PMMG_copyMetricsAndFields_point), surface if MG_BDY, volume otherwise.  The
 * class of a point depends only on its tags and on whether a valid tetra
 * references it, so the loop runs as two parallel passes: mark the
 * referenced points (every writer stores the same byte), then classify. */

typedef struct {
  const pmmg_new_group *g;
  uint8_t *pclass;
  int64_t k0, k1; /* tetra range (pass 1) / point range (pass 2) */
  int64_t count;
} cls_job;

static void *cls_mark(void *arg) {
  cls_job *J = (cls_job *)arg;
  const pmmg_new_group *g = J->g;
  for (int64_t k = J->k0; k < J->k1; k++) {
    const int *v = g->tetv + 4 * k;
    if (v[0] <= 0) continue; /* !MG_EOK */
    for (int l = 0; l < 4; l++)
      if (v[l] >= 1 && v[l] <= g->np) J->pclass[v[l] - 1] = 1;
  }
  return NULL;
}

static void *cls_assign(void *arg) {
  cls_job *J = (cls_job *)arg;
  const pmmg_new_group *g = J->g;
  int64_t n = 0;
  for (int64_t i = J->k0; i < J->k1; i++) {
    if (!J->pclass[i]) continue;
    uint16_t tag = g->tag ? g->tag[i] : 0;
    if (tag >= PMMG_TAG_NUL || (tag & PMMG_TAG_REQ)) {
      J->pclass[i] = PMMG_PT_SKIP;
      continue;
    }
    J->pclass[i] = (tag & PMMG_TAG_BDY) ? PMMG_PT_BDY : PMMG_PT_VOL;
    n++;
  }
  J->count = n;
  return NULL;
}

static int host_threads(void) {
  long n = sysconf(_SC_NPROCESSORS_ONLN);
  const char *e = getenv("PMMG_HOST_THREADS");
  if (e && atoi(e) > 0) n = atoi(e);
  if (n < 1) n = 1;
  if (n > 16) n = 16;
  return (int)n;
}

int64_t pmmg_classify_points(const pmmg_new_group *g, uint8_t *pclass) {
  memset(pclass, PMMG_PT_SKIP, (size_t)g->np);
  int nt = host_threads();
  cls_job J[16];
  pthread_t th[16];
  for (int pass = 0; pass < 2; pass++) {
    const int64_t n = pass == 0 ? (int64_t)g->ne : (int64_t)g->np;
    for (int t = 0; t < nt; t++) {
      J[t].g = g;
      J[t].pclass = pclass;
      J[t].k0 = n * t / nt;
      J[t].k1 = n * (t + 1) / nt;
      J[t].count = 0;
      if (pthread_create(&th[t], NULL, pass == 0 ? cls_mark : cls_assign, &J[t]) != 0) {
        (pass == 0 ? cls_mark : cls_assign)(&J[t]);
        th[t] = 0;
      }
    }
    for (int t = 0; t < nt; t++)
      if (th[t]) pthread_join(th[t], NULL);
  }
  int64_t total = 0;
  for (int t = 0; t < nt; t++) total += J[t].count;
  return total;
}

/* ---------------------------------------------------------------- frozen points */

static int copy_sol_point(const pmmg_old_group *old, int size, const double *src, double *dst, int np_new,
                          const int *perm) {
  /* PMMG_copySol_point, src/interpmesh_pmmg.c:311-358 */
  for (int ip = 1; ip <= old->np; ip++) {
    uint16_t tag = old->tag[ip - 1];
    if (tag >= PMMG_TAG_NUL) continue; /* !MG_VOK */
    if (!(tag & PMMG_TAG_REQ)) continue;
    int to = perm ? perm[ip] : ip;
    if (to < 1 || to > np_new) return 0;
    memcpy(dst + (size_t)size * (to - 1), src + (size_t)size * (ip - 1), sizeof(double) * (size_t)size);
  }
  return 1;
}

int pmmg_copy_metrics_and_fields_point(const pmmg_old_group *old, pmmg_new_group *g, const int *permNodGlob,
                                       int renum, int input_met) {
  if (!old || !g || !old->tag) return 0;
  /* no permutation array, or no renumbering: the same index (:321-337) */
  const int *perm = (renum && permNodGlob) ? permNodGlob : NULL;
  /* PMMG_copyMetrics_point, src/interpmesh_pmmg.c:373-383 */
  if (input_met == 1 && !(g->hsiz > 0.0) && old->met_size > 0) {
    if (!g->met || g->met_size != old->met_size) return 0;
    if (!copy_sol_point(old, old->met_size, old->met, g->met, g->np, perm)) return 0;
  }
  /* PMMG_copyFields_point, :397-415 */
  for (int j = 0; j < old->nfield; j++)
    if (!copy_sol_point(old, old->field_size[j], old->field[j], g->field[j], g->np, perm)) return 0;
  return 1;
}

int pmmg_set_constant_metric(pmmg_new_group *g) {
  /* MMG3D_Set_constantSize: met->size from info.ani; MMG5_Compute_constantSize
   * (Mmg @889d408, not in the reference tree: parity unpinned) rejects a
   * uniform size outside the user bounds ("Mismatched options: hmin ... is
   * greater than hsiz" / "hmax ... is lower than hsiz"), and
   * PMMG_interpMetricsAndFields_mesh then fails (src/interpmesh_pmmg.c:504);
   * MMG5_Set_constantSize: valid points only */
  const int size = g->ani ? 6 : 1;
  if (!g->met || g->met_size != size || !(g->hsiz > 0.0)) return 0;
  const double h = g->hsiz;
  if ((g->hmin > 0.0 && g->hmin > h) || (g->hmax > 0.0 && g->hmax < h)) {
    fprintf(stderr, "[parmmg_host] mismatched options: hmin (%e), hmax (%e), hsiz (%e)\n", g->hmin, g->hmax, h);
    return 0;
  }
  const double isq = 1.0 / (h * h);
  for (int i = 0; i < g->np; i++) {
    if (g->tag && g->tag[i] >= PMMG_TAG_NUL) continue; /* !MG_VOK */
    double *m = g->met + (size_t)size * i;
    if (size == 1) {
      m[0] = h;
    } else {
      m[0] = isq; m[1] = 0.0; m[2] = 0.0; m[3] = isq; m[4] = 0.0; m[5] = isq;
    }
  }
  return 1;
}

/* 1 with a context; else 0, after the message of an entry point (`what`) that has nothing to run on */
static int have_ctx(const pmmg_hip_ctx *ctx, const char *what) {
  if (!ctx) fprintf(stderr, "[parmmg_host] no HIP context: %s has no CPU fallback\n", what);
  return ctx != NULL;
}

static void stats_add(pmmg_hip_stats *a, const pmmg_hip_stats *b) {
  a->nvol += b->nvol; a->nbdy += b->nbdy;
  a->nvol_walk += b->nvol_walk; a->nvol_exhaust += b->nvol_exhaust; a->nvol_closest += b->nvol_closest;
  a->nvol_exact += b->nvol_exact;
  a->nbdy_face += b->nbdy_face; a->nbdy_edge += b->nbdy_edge; a->nbdy_vertex += b->nbdy_vertex;
  a->nbdy_wedge += b->nbdy_wedge; a->nbdy_cone += b->nbdy_cone; a->nbdy_exhaust += b->nbdy_exhaust;
  a->nbdy_stale += b->nbdy_stale; a->nbdy_closest += b->nbdy_closest;
  a->steps_total += b->steps_total;
  a->wave_iters += b->wave_iters;
  if (b->stepmax > a->stepmax) a->stepmax = b->stepmax;
  a->ms_prepare += b->ms_prepare; a->ms_sort += b->ms_sort; a->ms_vol += b->ms_vol; a->ms_bdy += b->ms_bdy;
  a->ms_fallback += b->ms_fallback; a->ms_total += b->ms_total; a->ms_vol_locate += b->ms_vol_locate;
  a->nvol_noseed += b->nvol_noseed; a->nvol_stuck += b->nvol_stuck; a->nvol_limit += b->nvol_limit;
  a->seed_map_axes |= b->seed_map_axes;
  a->nbdy_fanscan += b->nbdy_fanscan;
  a->nvol_src += b->nvol_src; a->nbdy_src += b->nbdy_src;
}

static int interp_groups(pmmg_hip_ctx *ctx, int ngrp, const pmmg_old_group *old, pmmg_new_group *grp, int input_met,
                         int keep, int carried, const int *const *src, const int *const *pmap,
                         pmmg_hip_stats *stats) {
  if (!have_ctx(ctx, "the transfer step")) return 0;
  if (stats) memset(stats, 0, sizeof(*stats));
  int ier = 1;
  for (int ig = 0; ig < ngrp; ig++) {
    const pmmg_old_group *o = &old[ig];
    pmmg_new_group *g = &grp[ig];
    /* ismet logic, src/interpmesh_pmmg.c:497-512 */
    int ismet = 1;
    if (input_met != 1) {
      ismet = 0;
    } else if (g->hsiz > 0.0) {
      if (!pmmg_set_constant_metric(g)) {
        if (keep) pmmg_hip_carry_over(ctx, ig, 0, NULL);
        ier = 0;
        continue;
      }
      ismet = 0;
    }
    /* a group left out drops what was kept for it (its next old group is
     * not this call's output) */
    if (!ismet && o->nfield == 0) { /* nothing to do */
      if (keep) pmmg_hip_carry_over(ctx, ig, 0, NULL);
      continue;
    }
    if (ismet && (o->met_size == 0 || g->met_size != o->met_size || !g->met)) {
      if (keep) pmmg_hip_carry_over(ctx, ig, 0, NULL);
      ier = 0;
      continue;
    }
    uint8_t *pclass = (uint8_t *)malloc((size_t)g->np + 1);
    if (!pclass) { ier = 0; continue; }
    pmmg_classify_points(g, pclass);
    /* the previous iteration's new group ig, kept on the device: carried
     * unless nothing was kept for it (then it goes up whole) */
    if (carried && !pmmg_hip_carry_over(ctx, ig, o->np, src ? src[ig] : NULL))
      fprintf(stderr, "[parmmg_host] group %d: no carry-over (%s), uploading it\n", ig, pmmg_hip_last_error(ctx));
    /* the background: adjacency and boundary trias are built on the device
     * when the caller does not hand them over (set_background, adja / triv
     * NULL) */
    int ok = pmmg_hip_set_background(ctx, o->np, o->xyz, o->ne, o->tetv, o->adja, o->nt, o->triv, o->adjt,
                                     o->hausd, PMMG_HIP_HOST) &&
             pmmg_hip_set_solutions(ctx, ismet ? o->met_size : 0, ismet ? o->met : NULL, o->nfield,
                                    o->field_size, o->field, PMMG_HIP_HOST);
    /* USE_POINTMAP: the group's MMG5_Point.src arms the call (pmmg_hip_set_point_map) */
    if (ok && pmap && pmap[ig]) ok = pmmg_hip_set_point_map(ctx, g->np, pmap[ig], PMMG_HIP_HOST);
    pmmg_hip_stats st;
    if (ok)
      ok = pmmg_hip_locate_interp(ctx, g->np, g->xyz, pclass, ismet ? g->met : NULL, g->field, g->elem, g->hit,
                                  &st, PMMG_HIP_HOST);
    if (ok && stats) stats_add(stats, &st);
    if (ok && keep) ok = pmmg_hip_keep(ctx, ig);
    if (!ok && keep) pmmg_hip_carry_over(ctx, ig, 0, NULL);
    if (!ok) ier = 0;
    free(pclass);
  }
  return ier;
}

int pmmg_interp_metrics_and_fields(pmmg_hip_ctx *ctx, int ngrp, const pmmg_old_group *old, pmmg_new_group *grp,
                                   int input_met, pmmg_hip_stats *stats) {
  return interp_groups(ctx, ngrp, old, grp, input_met, 0, 0, NULL, NULL, stats);
}

int pmmg_interp_metrics_and_fields_map(pmmg_hip_ctx *ctx, int ngrp, const pmmg_old_group *old, pmmg_new_group *grp,
                                       int input_met, const int *const *src, pmmg_hip_stats *stats) {
  if (!ctx || !old || !grp) return 0;
  return interp_groups(ctx, ngrp, old, grp, input_met, 0, 0, NULL, src, stats);
}

int pmmg_interp_metrics_and_fields_carry(pmmg_hip_ctx *ctx, int ngrp, const pmmg_old_group *old,
                                         pmmg_new_group *grp, int input_met, int carried, const int *const *src,
                                         pmmg_hip_stats *stats) {
  return interp_groups(ctx, ngrp, old, grp, input_met, 1, carried, src, NULL, stats);
}

/* ---------------------------------------------------------------- METIS element graph */

void pmmg_host_free(void *p) { free(p); }

int pmmg_graph_mesh_elts2metis(pmmg_hip_ctx *ctx, int np, const double *xyz, int ne, const int *tetv, const int *adja,
                               int met_size, const double *met, int want_wgt, int **xadj, int **adjncy, int **adjwgt,
                               int64_t *nadjncy) {
  if (!have_ctx(ctx, "the element graph")) return 0;
  if (!xadj || !adjncy || !adjwgt || !nadjncy || np < 0 || ne < 0 || (ne > 0 && !tetv) ||
      (want_wgt && ne > 0 && !xyz) || ne >= (1 << 29))
    return 0;
  *xadj = *adjncy = *adjwgt = NULL;
  *nadjncy = 0;
  if (!met) met_size = 0; /* no metric: PMMG_computeWgt gives PMMG_WGTVAL_HUGEINT */
  const int wgt = want_wgt != 0;
  const int64_t cap = 4 * (int64_t)ne; /* device arrays for every face; the host ones are sized from the count */
  const int64_t i4 = (int64_t)sizeof(int), d8 = (int64_t)sizeof(double);
  int *h_xadj = NULL, *h_adj = NULL, *h_wgt = NULL;
  pmmg_stage st = pmmg_stage_begin(ctx);
  const int *d_tetv = pmmg_stage_up(&st, tetv, i4 * 4 * ne), *d_adja = pmmg_stage_up(&st, adja, i4 * 4 * ne);
  const double *d_xyz = wgt ? pmmg_stage_up(&st, xyz, d8 * 3 * np) : NULL;
  const double *d_met = wgt ? pmmg_stage_up(&st, met, d8 * met_size * np) : NULL;
  int *d_xadj = pmmg_stage_room(&st, i4 * ((int64_t)ne + 1)), *d_adj = pmmg_stage_room(&st, i4 * cap);
  int *d_wgt = wgt ? pmmg_stage_room(&st, i4 * cap) : NULL;
  int64_t n = 0;
  int ok = st.ok && pmmg_hip_metis_graph(ctx, np, d_xyz, ne, d_tetv, d_adja, NULL, met_size, d_met, (int)cap, &n,
                                         d_xadj, d_adj, d_wgt);
  if (ok) {
    /* (the reference allocates one entry more than the count, src/metis_pmmg.c:783: never empty) */
    h_xadj = (int *)malloc(sizeof(int) * ((size_t)ne + 1));
    h_adj = (int *)calloc((size_t)n + 1, sizeof(int));
    if (wgt) h_wgt = (int *)calloc((size_t)n + 1, sizeof(int));
    ok = h_xadj && h_adj && (!wgt || h_wgt) &&
         pmmg_hip_memcpy_d2h(ctx, h_xadj, d_xadj, (int64_t)sizeof(int) * ((int64_t)ne + 1)) &&
         pmmg_hip_memcpy_d2h(ctx, h_adj, d_adj, (int64_t)sizeof(int) * n) &&
         (!wgt || pmmg_hip_memcpy_d2h(ctx, h_wgt, d_wgt, (int64_t)sizeof(int) * n));
  }
  pmmg_stage_end(&st);
  if (!ok) {
    free(h_xadj);
    free(h_adj);
    free(h_wgt);
    return 0;
  }
  *xadj = h_xadj;
  *adjncy = h_adj;
  *adjwgt = h_wgt;
  *nadjncy = n;
  return 1;
}

/* ---------------------------------------------------------------- contiguity of a partition */

int pmmg_check_part_contiguity(pmmg_hip_ctx *ctx, int ne, const int *tetv, const int *adja, const int *part, int ncolor,
                               int *ncomp) {
  if (!have_ctx(ctx, "the contiguity check")) return -1;
  if (ne < 0 || ncolor < 1 || !ncomp || (ne > 0 && !tetv && !adja)) return -1;
  const int64_t i4 = (int64_t)sizeof(int);
  pmmg_stage st = pmmg_stage_begin(ctx);
  const int *d_tetv = pmmg_stage_up(&st, tetv, i4 * 4 * ne), *d_adja = pmmg_stage_up(&st, adja, i4 * 4 * ne);
  const int *d_part = pmmg_stage_up(&st, part, i4 * ne);
  int64_t nsub = 0;
  int ok = st.ok;
  /* the table itself is not wanted, but a call without room for it returns 0: give it room, once more when the
   * first guess was too small (the call then left *nsub, and only that refusal leaves it above cap) */
  int64_t cap = ne < 4096 ? ne : 4096;
  pmmg_hip_subgroup *sub = NULL;
  for (int turn = 0; ok && turn < 2; turn++) {
    sub = (pmmg_hip_subgroup *)malloc(sizeof(pmmg_hip_subgroup) * (size_t)(cap > 0 ? cap : 1));
    if (!sub) {
      ok = 0;
      break;
    }
    nsub = 0;
    ok = pmmg_hip_part_subgroups(ctx, ne, d_tetv, d_adja, NULL, d_part, ncolor, NULL, NULL, ncomp, (int)cap, sub, &nsub,
                                 NULL);
    free(sub);
    if (ok || turn == 1 || nsub <= cap) break;
    cap = nsub;
    ok = 1;
  }
  pmmg_stage_end(&st);
  return ok ? ncomp[ncolor - 1] : -1;
}

int pmmg_fix_contiguity_split(pmmg_hip_ctx *ctx, int ne, const int *tetv, const int *adja, int ngrp, int *part) {
  if (!have_ctx(ctx, "the contiguity fix")) return 0;
  if (ne < 0 || ngrp < 1 || (ne > 0 && (!part || (!tetv && !adja)))) return 0;
  if (ne == 0) return 1;
  const int64_t i4 = (int64_t)sizeof(int);
  int64_t nmoved = 0;
  int nmerged = 0, nstuck = 0;
  pmmg_stage st = pmmg_stage_begin(ctx);
  const int *d_tetv = pmmg_stage_up(&st, tetv, i4 * 4 * ne), *d_adja = pmmg_stage_up(&st, adja, i4 * 4 * ne);
  int *d_part = pmmg_stage_up(&st, part, i4 * ne);
  int ok = st.ok && pmmg_hip_fix_contiguity(ctx, ne, d_tetv, d_adja, NULL, d_part, ngrp, &nmoved, &nmerged, &nstuck);
  if (ok && nmerged) ok = pmmg_hip_memcpy_d2h(ctx, part, d_part, i4 * ne);
  pmmg_stage_end(&st);
  return ok;
}


/* ---------------------------------------------------------------- interface displacement */

int pmmg_part_move_interfaces(pmmg_hip_ctx *ctx, int np, int ne, const int *tetv, const int *adja, const int *mark,
                              int ncolor, const int *weight, const int *nelem_local, int nlayers, int *part_out,
                              int *layers_done, int *blocked) {
  if (!have_ctx(ctx, "the interface displacement")) return 0;
  if (np < 0 || ne < 0 || ncolor < 1 || nlayers < 0 || !weight || !nelem_local ||
      (ne > 0 && (!tetv || !mark || !part_out)))
    return 0;
  int done = 0, blk = 0;
  if (layers_done) *layers_done = 0;
  if (blocked) *blocked = 0;
  if (ne == 0) return 1;
  int *nelem = (int *)malloc(sizeof(int) * (size_t)ncolor * 2), *moved = (int *)malloc(sizeof(int) * (size_t)(nlayers + 1));
  const int64_t i4 = (int64_t)sizeof(int);
  pmmg_stage st = pmmg_stage_begin(ctx);
  int ok = nelem && moved;
  if (ok) {
    int *nemin = nelem + ncolor;
    for (int g = 0; g < ncolor; g++) {
      nelem[g] = nelem_local[g];
      const int half = nelem[g] / 2 + 1;
      nemin[g] = nelem[g] < 0 ? 0 : (half < 6 ? half : 6); /* MG_MIN(PMMG_REDISTR_NELEM_MIN, negrp/2+1) */
    }
    const int *d_tetv = pmmg_stage_up(&st, tetv, i4 * 4 * ne), *d_adja = pmmg_stage_up(&st, adja, i4 * 4 * ne);
    int *d_mark = pmmg_stage_up(&st, mark, i4 * ne), *color = pmmg_stage_room(&st, i4 * np);
    unsigned char *front = pmmg_stage_room(&st, np);
    ok = st.ok && pmmg_hip_ifc_seed(ctx, np, ne, d_tetv, NULL, d_mark, ncolor, weight, color, front);
    if (ok)
      ok = pmmg_hip_ifc_layers(ctx, np, ne, d_tetv, NULL, d_mark, ncolor, weight, nelem, nemin, color, front, 0, NULL,
                               NULL, nlayers, &done, &blk, moved);
    if (ok && !blk) {
      int64_t nmoved = 0;
      int nmerged = 0, nstuck = 0;
      ok = pmmg_hip_fix_contiguity(ctx, ne, d_tetv, d_adja, NULL, d_mark, ncolor, &nmoved, &nmerged, &nstuck);
    }
    if (ok) ok = pmmg_hip_memcpy_d2h(ctx, part_out, d_mark, i4 * ne);
  }
  if (ok && layers_done) *layers_done = done;
  if (ok && blocked) *blocked = blk;
  pmmg_stage_end(&st);
  free(nelem);
  free(moved);
  return ok;
}


/* ---------------------------------------------------------------- group split */

void pmmg_split_result_free(pmmg_split_result *r) {
  if (!r) return;
  void *p[] = {r->count, r->old_tet, r->new_tet, r->tetv, r->adja, r->old_pt, r->xyz, r->met,
               r->face_idx1, r->face_idx2, r->node_idx1, r->node_idx2};
  for (size_t i = 0; i < sizeof(p) / sizeof(p[0]); i++) free(p[i]);
  if (r->fields)
    for (int i = 0; i < r->nfield; i++) free(r->fields[i]);
  free(r->fields);
  memset(r, 0, sizeof(*r));
}

int pmmg_split_grps(pmmg_hip_ctx *ctx, int np, const double *xyz, int ne, const int *tetv, const int *adja,
                    const int *part, int ngrp, int met_size, const double *met, int nfield, const int *field_size,
                    const double *const *fields, const int *node_pos, const int *face_old, int nnode0, int nface0,
                    pmmg_split_result *out) {
  if (!have_ctx(ctx, "the group split")) return 0;
  if (!out) return 0;
  memset(out, 0, sizeof(*out));
  if (np < 0 || ne < 0 || ngrp < 1 || nfield < 0 || (nfield > 0 && (!field_size || !fields)) ||
      (ne > 0 && (!xyz || !tetv || !adja || !part)))
    return 0;
  if (!met) met_size = 0;
  const int64_t nt = ne, i4 = (int64_t)sizeof(int), d8 = (int64_t)sizeof(double);
  pmmg_stage st = pmmg_stage_begin(ctx);
  const int *d_tetv = pmmg_stage_up(&st, tetv, i4 * 4 * nt), *d_adja = pmmg_stage_up(&st, adja, i4 * 4 * nt);
  const int *d_part = pmmg_stage_up(&st, part, i4 * nt), *d_npos = pmmg_stage_up(&st, node_pos, i4 * np);
  const int *d_fold = pmmg_stage_up(&st, face_old, i4 * 4 * nt);
  int *d_oldt = pmmg_stage_room(&st, i4 * nt), *d_newt = pmmg_stage_room(&st, i4 * nt);
  int *d_tv = pmmg_stage_room(&st, i4 * 4 * nt), *d_ad = pmmg_stage_room(&st, i4 * 4 * nt);
  out->count = (pmmg_hip_split_count *)calloc((size_t)ngrp, sizeof(pmmg_hip_split_count));
  if (!out->count) st.ok = 0;
  /* caps of 0 size the lists: that call returns 0 with the counts filled unless every list is empty */
  int sized = 0;
  if (st.ok)
    sized = pmmg_hip_split_groups(ctx, np, ne, d_tetv, d_adja, NULL, d_part, ngrp, d_npos, d_fold, nnode0, nface0,
                                  out->count, 0, 0, 0, d_oldt, d_newt, d_tv, d_ad, NULL, NULL, NULL, NULL, NULL, NULL,
                                  &out->nnode_end, &out->nface_end);
  int64_t tot_ne = 0;
  for (int g = 0; st.ok && g < ngrp; g++) {
    tot_ne += out->count[g].ne;
    out->npt += out->count[g].np;
    out->nface += out->count[g].nface;
    out->nnode += out->count[g].nnode;
  }
  if (!sized && tot_ne != nt) st.ok = 0; /* a refusal: the counts were left at 0 */
  int *d_oldp = pmmg_stage_room(&st, i4 * out->npt);
  int *d_f1 = pmmg_stage_room(&st, i4 * out->nface), *d_f2 = pmmg_stage_room(&st, i4 * out->nface);
  int *d_n1 = pmmg_stage_room(&st, i4 * out->nnode), *d_n2 = pmmg_stage_room(&st, i4 * out->nnode);
  if (st.ok && !sized)
    st.ok = pmmg_hip_split_groups(ctx, np, ne, d_tetv, d_adja, NULL, d_part, ngrp, d_npos, d_fold, nnode0, nface0,
                                  out->count, out->npt, out->nface, out->nnode, d_oldt, d_newt, d_tv, d_ad, NULL,
                                  d_oldp, d_f1, d_f2, d_n1, d_n2, &out->nnode_end, &out->nface_end);
  /* the point rows through old_pt: xyz, the metric, every field, one after the other through one device block */
  int width = met_size > 3 ? met_size : 3;
  for (int i = 0; i < nfield; i++)
    if (field_size[i] > width) width = field_size[i];
  const double *d_xyz = pmmg_stage_up(&st, xyz, d8 * 3 * np);
  double *rows = pmmg_stage_room(&st, d8 * width * out->npt);
  out->xyz = pmmg_stage_rows(&st, out->npt, d_oldp, 3, d_xyz, rows);
  if (met_size)
    out->met = pmmg_stage_rows(&st, out->npt, d_oldp, met_size, pmmg_stage_up(&st, met, d8 * met_size * np), rows);
  out->met_size = met_size;
  if (st.ok && nfield) {
    out->fields = (double **)calloc((size_t)nfield, sizeof(double *));
    if (out->fields)
      out->nfield = nfield;
    else
      st.ok = 0;
  }
  for (int i = 0; st.ok && i < nfield; i++) {
    if (field_size[i] < 1 || !fields[i]) {
      st.ok = 0;
      break;
    }
    const double *d_field = pmmg_stage_up(&st, fields[i], d8 * field_size[i] * np);
    out->fields[i] = pmmg_stage_rows(&st, out->npt, d_oldp, field_size[i], d_field, rows);
  }
  out->old_tet = pmmg_stage_down(&st, d_oldt, i4 * nt);
  out->new_tet = pmmg_stage_down(&st, d_newt, i4 * nt);
  out->tetv = pmmg_stage_down(&st, d_tv, i4 * 4 * nt);
  out->adja = pmmg_stage_down(&st, d_ad, i4 * 4 * nt);
  out->old_pt = pmmg_stage_down(&st, d_oldp, i4 * out->npt);
  out->face_idx1 = pmmg_stage_down(&st, d_f1, i4 * out->nface);
  out->face_idx2 = pmmg_stage_down(&st, d_f2, i4 * out->nface);
  out->node_idx1 = pmmg_stage_down(&st, d_n1, i4 * out->nnode);
  out->node_idx2 = pmmg_stage_down(&st, d_n2, i4 * out->nnode);
  pmmg_stage_end(&st);
  if (!st.ok) pmmg_split_result_free(out);
  return st.ok;
}

/* ---------------------------------------------------------------- group merge */

void pmmg_merge_result_free(pmmg_merge_result *r) {
  if (!r) return;
  void *p[] = {r->new_pt, r->src_pt, r->new_tet, r->src_tet, r->tetv, r->mark, r->tref, r->xyz, r->met, r->node_val,
               r->face_val};
  for (size_t i = 0; i < sizeof(p) / sizeof(p[0]); i++) free(p[i]);
  memset(r, 0, sizeof(*r));
}

int pmmg_merge_grps(pmmg_hip_ctx *ctx, int ngrp, const pmmg_hip_split_count *count, const int *tetv,
                    const int *node_idx1, const int *node_idx2, const int *face_idx1, const int *face_idx2, int nnode,
                    int nface, const int *color, const double *xyz, int met_size, const double *met, const int *tref,
                    pmmg_merge_result *out) {
  if (!have_ctx(ctx, "the group merge")) return 0;
  if (!out) return 0;
  memset(out, 0, sizeof(*out));
  if (ngrp < 1 || !count || nnode < 0 || nface < 0) return 0;
  int64_t nt = 0, npt = 0, nfe = 0, nne = 0;
  for (int g = 0; g < ngrp; g++) {
    if (count[g].ne < 0 || count[g].np < 0 || count[g].nface < 0 || count[g].nnode < 0) return 0;
    nt += count[g].ne;
    npt += count[g].np;
    nfe += count[g].nface;
    nne += count[g].nnode;
  }
  if ((nt > 0 && !tetv) || (npt > 0 && !xyz) || (nfe > 0 && (!face_idx1 || !face_idx2)) ||
      (nne > 0 && (!node_idx1 || !node_idx2)))
    return 0;
  if (!met) met_size = 0;
  const int64_t i4 = (int64_t)sizeof(int), d8 = (int64_t)sizeof(double);
  pmmg_stage st = pmmg_stage_begin(ctx);
  const int *d_tetv = pmmg_stage_up(&st, tetv, i4 * 4 * nt);
  const int *d_n1 = pmmg_stage_up(&st, node_idx1, i4 * nne), *d_n2 = pmmg_stage_up(&st, node_idx2, i4 * nne);
  const int *d_f1 = pmmg_stage_up(&st, face_idx1, i4 * nfe), *d_f2 = pmmg_stage_up(&st, face_idx2, i4 * nfe);
  int *d_newp = pmmg_stage_room(&st, i4 * npt), *d_newt = pmmg_stage_room(&st, i4 * nt);
  int *d_srcp = pmmg_stage_room(&st, i4 * npt); /* (the merged points are at most the groups') */
  int *d_srct = pmmg_stage_room(&st, i4 * nt), *d_tv = pmmg_stage_room(&st, i4 * 4 * nt);
  int *d_mark = color ? pmmg_stage_room(&st, i4 * nt) : NULL;
  int *d_nval = pmmg_stage_room(&st, i4 * nnode), *d_fval = pmmg_stage_room(&st, i4 * nface);
  if (st.ok)
    st.ok = pmmg_hip_merge_groups(ctx, ngrp, count, d_tetv, NULL, d_n1, d_n2, d_f1, d_f2, nnode, nface, color, npt,
                                  d_newp, d_newt, d_srcp, d_srct, d_tv, d_mark, d_nval, d_fval, &out->np, &out->ne);
  /* the point rows through src_pt and the references through src_tet, through one device block */
  const int width = met_size > 3 ? met_size : 3;
  const double *d_xyz = pmmg_stage_up(&st, xyz, d8 * 3 * npt);
  double *rows = pmmg_stage_room(&st, d8 * width * out->np);
  out->xyz = pmmg_stage_rows(&st, out->np, d_srcp, 3, d_xyz, rows);
  if (met_size)
    out->met = pmmg_stage_rows(&st, out->np, d_srcp, met_size, pmmg_stage_up(&st, met, d8 * met_size * npt), rows);
  out->met_size = met_size;
  if (tref) {
    const int *d_tref = pmmg_stage_up(&st, tref, i4 * nt);
    out->tref = pmmg_stage_rows_i32(&st, nt, d_srct, 1, d_tref, pmmg_stage_room(&st, i4 * nt));
  }
  out->new_pt = pmmg_stage_down(&st, d_newp, i4 * npt);
  out->src_pt = pmmg_stage_down(&st, d_srcp, i4 * out->np);
  out->new_tet = pmmg_stage_down(&st, d_newt, i4 * nt);
  out->src_tet = pmmg_stage_down(&st, d_srct, i4 * nt);
  out->tetv = pmmg_stage_down(&st, d_tv, i4 * 4 * nt);
  if (color) out->mark = pmmg_stage_down(&st, d_mark, i4 * nt);
  out->node_val = pmmg_stage_down(&st, d_nval, i4 * nnode);
  out->face_val = pmmg_stage_down(&st, d_fval, i4 * nface);
  pmmg_stage_end(&st);
  if (!st.ok) pmmg_merge_result_free(out);
  return st.ok;
}
