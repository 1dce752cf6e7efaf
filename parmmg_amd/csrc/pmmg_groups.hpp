// pmmg_groups.hpp — many groups in one call (included by pmmg_hip.hip only):
// the lanes of pmmg_hip_locate_interp_groups, each a context of its own that
// runs its share of the groups through the ordinary entry points.
#pragma once

#include <string>

#include "pmmg_call.hpp" // collect_stats

// ---- many groups in one call

static void stats_sum(pmmg_hip_stats *a, const pmmg_hip_stats &b) {
  a->nvol += b.nvol; a->nbdy += b.nbdy;
  a->nvol_walk += b.nvol_walk; a->nvol_exhaust += b.nvol_exhaust; a->nvol_closest += b.nvol_closest;
  a->nvol_exact += b.nvol_exact;
  a->nbdy_face += b.nbdy_face; a->nbdy_edge += b.nbdy_edge; a->nbdy_vertex += b.nbdy_vertex;
  a->nbdy_wedge += b.nbdy_wedge; a->nbdy_cone += b.nbdy_cone; a->nbdy_exhaust += b.nbdy_exhaust;
  a->nbdy_stale += b.nbdy_stale; a->nbdy_closest += b.nbdy_closest;
  a->steps_total += b.steps_total; a->wave_iters += b.wave_iters;
  a->sorted += b.sorted; // the number of groups whose queries were Morton-binned
  if (b.stepmax > a->stepmax) a->stepmax = b.stepmax;
  a->ms_prepare += b.ms_prepare; a->ms_sort += b.ms_sort; a->ms_vol += b.ms_vol; a->ms_bdy += b.ms_bdy;
  a->ms_fallback += b.ms_fallback; a->ms_total += b.ms_total; a->ms_vol_locate += b.ms_vol_locate;
  a->nvol_noseed += b.nvol_noseed; a->nvol_stuck += b.nvol_stuck; a->nvol_limit += b.nvol_limit;
  a->seed_map_axes |= b.seed_map_axes;
  a->nbdy_fanscan += b.nbdy_fanscan;
  a->nvol_src += b.nvol_src; a->nbdy_src += b.nbdy_src;
}

static pmmg_hip_ctx *group_lane(pmmg_hip_ctx *c, int j) {
  while ((int)c->lanes.size() <= j) {
    const bool first = c->lanes.empty();
    pmmg_hip_ctx *l = create_ctx(c->device, c->options, first ? c : nullptr);
    if (!l) {
      set_err(c, "locate_interp_groups: cannot create group lane %d", (int)c->lanes.size());
      return nullptr;
    }
    if (!l->borrowed_streams) { // one stream per lane (pmmg_hip_ctx::group_lanes: the hardware's 4 queues)
      (void)hipStreamDestroy(l->stream2);
      l->stream2 = l->stream;
    }
    c->lanes.push_back(l);
  }
  return c->lanes[j];
}

// one lane's share of a groups call: groups j, j + L, j + 2L, ... enqueued in
// order (each waited for and its counters summed when stats are wanted)
static int lane_groups(pmmg_hip_ctx *l, int j, int L, int ngroup, const pmmg_hip_group *groups, bool want,
                       pmmg_hip_stats *sum, int *bad) {
  if (hipSetDevice(l->device) != hipSuccess) {
    *bad = j;
    return 0;
  }
  for (int i = j; i < ngroup; i += L) {
    const pmmg_hip_group &g = groups[i];
    const int ok =
        (g.tet8 ? pmmg_hip_set_background_tet8(l, g.np, g.xyz, g.ne, g.tet8, g.nt, g.triv, g.adjt, g.hausd,
                                               PMMG_HIP_DEVICE)
                : (g.tetv && pmmg_hip_set_background(l, g.np, g.xyz, g.ne, g.tetv, g.adja, g.nt, g.triv, g.adjt,
                                                     g.hausd, PMMG_HIP_DEVICE))) &&
        pmmg_hip_set_solutions(l, g.met_size, g.met, g.nfield, g.field_size, g.fields, PMMG_HIP_DEVICE) &&
        pmmg_hip_locate_interp(l, g.np_new, g.xyz_new, g.pclass, g.met_out, g.fields_out, g.elem_out, g.hit_out,
                               nullptr, PMMG_HIP_DEVICE);
    pmmg_hip_stats st;
    if (!ok || (want && (hipStreamSynchronize(l->stream) != hipSuccess || !collect_stats(l, &st)))) {
      *bad = i;
      return 0;
    }
    if (want) stats_sum(sum, st);
  }
  return 1;
}

// pmmg_hip_locate_interp_groups on a context: the groups dealt to the lanes and enqueued
static int groups_call(pmmg_hip_ctx *c, int ngroup, const pmmg_hip_group *groups, pmmg_hip_stats *stats) {
  if (stats) memset(stats, 0, sizeof(*stats));
  if (ngroup <= 0) return 1;
  if (!groups) {
    set_err(c, "locate_interp_groups: groups is NULL");
    return 0;
  }
  if (!enter(c)) return 0;
  // a large call's extra streams (binning, refill) are released before the lanes take theirs, so that the
  // lanes' streams find the queues those held (a later large call creates them again)
  for (hipStream_t *x : {&c->stream3, &c->stream_f})
    if (*x && c->lanes.size() < (size_t)std::min(c->group_lanes, ngroup)) {
      HIPCK(c, hipStreamSynchronize(*x));
      HIPCK(c, hipStreamDestroy(*x));
      *x = nullptr;
    }
  // lanes dealt an equal number of groups: ceil(n / rounds) lanes for the rounds the most lanes need
  // (10 groups, 5 lanes: 2 each; 7 groups: 4 lanes of 2, 2, 2, 1 rather than 5 of 2, 2, 1, 1, 1)
  const int Lmax = std::max(1, c->group_lanes), rounds = (ngroup + Lmax - 1) / Lmax;
  const int L = std::max(1, std::min(ngroup, (ngroup + rounds - 1) / rounds));
  std::vector<pmmg_hip_ctx *> lane(L);
  for (int j = 0; j < L; j++)
    if (!(lane[j] = group_lane(c, j))) return 0;
  // every lane enqueues its groups from its own host thread (the enqueue of
  // ~25 launches per group is the host's share of a small group)
  std::vector<pmmg_hip_stats> sums(L);
  std::vector<int> bad(L, -1), ok(L, 1);
  for (auto &x : sums) memset(&x, 0, sizeof(x));
  if (L > 1 && !c->lane_pool) c->lane_pool = new Pool(c->group_lanes - 1);
  auto work = [&](size_t a, size_t e) {
    for (size_t j = a; j < e; j++)
      ok[j] = lane_groups(lane[j], (int)j, L, ngroup, groups, stats != nullptr, &sums[j], &bad[j]);
  };
  if (L > 1) c->lane_pool->run((size_t)L, (size_t)L, work);
  else work(0, 1);
  HIPCK(c, hipSetDevice(c->device));
  int first = -1, fl = 0;
  for (int j = 0; j < L; j++)
    if (!ok[j] && (first < 0 || bad[j] < first)) {
      first = bad[j];
      fl = j;
    }
  if (first >= 0) {
    const std::string why = lane[fl]->err;
    set_err(c, "locate_interp_groups: group %d: %s", first, why.c_str());
    return 0;
  }
  if (stats)
    for (int j = 0; j < L; j++) stats_sum(stats, sums[j]);
  return 1;
}
