"""A/B of the point map (pmmg_hip_set_point_map) against the seed grids, in
device mode, one process, one live context:

  python3 tools/gpu_job.py --tag r07a "py tools/point_map_ab.py --out bench_out/r07a/point_map.json"

Per config (cfg3, cfg4): one plain call gives the located elements; two maps
are derived from them on the host (parmmg_amd.synth.point_map) — `near`, the
nearest of the element's vertices, and `stale`, a random one of them — and,
after a warm-up, plain / near / stale calls alternate for --rounds rounds on
the same background.  Reported per variant (medians, and min / max of
ms_total): ms_prepare, ms_vol, ms_vol_locate, ms_bdy, ms_total, steps_total,
stepmax, lockstep efficiency steps_total / (64 wave_iters), the counters; and
the one-off cost of the start tables (pmmg_hip_start_elements after
pmmg_hip_release_scratch, against the same call with the tables in place).

Checked on the fly: wherever the plain call's volume walk accepted a tetra
with min barycentric coordinate > EPS (the point lies strictly inside one
tetra, class (i) of tests/parity.py), the mapped calls report the same
element and bit-equal rows; the count of points whose elements differ at all
is reported."""
import argparse
import ctypes
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from parmmg_amd import configs, synth  # noqa: E402
from parmmg_amd.transfer import DEVICE, TransferContext, pack_tet8  # noqa: E402

EPS = 1e-6  # MMG5_EPS
TIMES = ["ms_prepare", "ms_vol", "ms_vol_locate", "ms_bdy", "ms_total"]
COUNTS = ["steps_total", "stepmax", "wave_iters", "nvol", "nbdy", "nvol_src", "nbdy_src", "nvol_exact", "nvol_noseed",
          "nvol_exhaust", "nbdy_exhaust", "sorted"]


def min_bary(bg, xyz, elem, idx, chunk=1 << 21):
    """min barycentric coordinate of points idx in their located tetra"""
    out = np.empty(idx.size)
    for a in range(0, idx.size, chunk):
        ii = idx[a:a + chunk]
        p = bg.xyz[bg.tetv[elem[ii] - 1] - 1]  # (m, 4, 3)
        x = xyz[ii]
        d = p[:, 1:] - p[:, :1]
        vol = np.einsum("ij,ij->i", d[:, 0], np.cross(d[:, 1], d[:, 2]))
        lam = np.empty((ii.size, 4))
        for f in range(4):
            q = p.copy()
            q[:, f] = x
            e = q[:, 1:] - q[:, :1]
            lam[:, f] = np.einsum("ij,ij->i", e[:, 0], np.cross(e[:, 1], e[:, 2])) / vol
        out[a:a + chunk] = lam.min(axis=1)
    return out


def run_config(name, rounds, warmup):
    w = configs.SHORT[name]
    t0 = time.time()
    bg, new = configs.build_meshes(w)
    met = synth.solution(w.metric, bg.xyz)
    fields = [synth.solution(f, bg.xyz) for f in w.fields]
    pc = synth.classes(new)
    n = new.np
    print(f"[{name}] meshes in {time.time() - t0:.1f} s: {bg.ne} tetra, {bg.np} vertices, {bg.nt} trias, {n} new points",
          flush=True)
    res = {"config": w.name, "ne": bg.ne, "np": bg.np, "nt": bg.nt, "np_new": n, "rounds": rounds}
    with TransferContext(0) as ctx:
        d = dict(xyz=ctx.upload(bg.xyz), tet8=ctx.upload(pack_tet8(bg.tetv, bg.adja)), triv=ctx.upload(bg.triv),
                 adjt=ctx.upload(bg.adjt), met=ctx.upload(met), f=[ctx.upload(f) for f in fields],
                 q=ctx.upload(new.xyz), pc=ctx.upload(pc))
        ctx.set_background_tet8(d["xyz"], d["tet8"], d["triv"], d["adjt"], w.hausd)
        ctx.set_solutions(d["met"], d["f"])

        def outputs():
            return dict(mo=ctx.empty((n, w.met_size), np.float64),
                        fo=[ctx.empty((n, f.shape[1]), np.float64) for f in fields],
                        el=ctx.empty((n,), np.int32), hit=ctx.empty((n,), np.int8))

        out = {"plain": outputs()}

        def call(variant):
            o = out[variant]
            if variant != "plain":
                ctx.set_point_map(maps[variant])
            ctx.locate_interp(d["q"], d["pc"], o["mo"], o["fo"], o["el"], o["hit"], sync=False)
            return ctx.sync()

        maps = {}
        st = call("plain")
        elem, hit = out["plain"]["el"].download(), out["plain"]["hit"].download()
        t0 = time.time()
        host_maps = {"near": synth.point_map(bg, new.xyz, elem, pc),
                     "stale": synth.point_map(bg, new.xyz, elem, pc, stale=True)}
        print(f"[{name}] maps derived on the host in {time.time() - t0:.1f} s", flush=True)
        for k, m in host_maps.items():
            maps[k] = ctx.upload(m)
            out[k] = outputs()
        variants = ["plain", "near", "stale"]

        # the one-off start tables: built by start_elements after release_scratch, against the copy alone
        tab = [ctx.empty((bg.np,), np.int32), ctx.empty((bg.np,), np.int32)]
        build, copy = [], []
        for _ in range(3):
            for lst, release in ((build, True), (copy, False)):
                if release:
                    ctx.release_scratch()
                t0 = time.perf_counter()
                ok = ctx.lib.pmmg_hip_start_elements(ctx.h, ctypes.c_void_p(tab[0].ptr), ctypes.c_void_p(tab[1].ptr),
                                                     DEVICE)
                lst.append(1e3 * (time.perf_counter() - t0))
                if not ok:
                    raise RuntimeError(ctx.error())
        res["start_tables_ms"] = {"build_and_copy": build, "copy_only": copy,
                                  "build": round(float(np.median(build) - np.median(copy)), 4)}
        print(f"[{name}] start tables: {res['start_tables_ms']}", flush=True)

        for _ in range(warmup):
            for v in variants:
                call(v)
        rec = {v: {k: [] for k in TIMES + COUNTS} for v in variants}
        for r in range(rounds):
            for v in variants:  # alternating
                st = call(v)
                for k in TIMES + COUNTS:
                    rec[v][k].append(float(getattr(st, k)))
        res["variants"] = {}
        for v in variants:
            s = {k: round(float(np.median(rec[v][k])), 4) for k in TIMES}
            s.update({k: int(np.median(rec[v][k])) for k in COUNTS})
            s["ms_total_min"], s["ms_total_max"] = round(min(rec[v]["ms_total"]), 4), round(max(rec[v]["ms_total"]), 4)
            s["ms_total_series"] = [round(x, 4) for x in rec[v]["ms_total"]]
            s["lockstep_efficiency"] = round(s["steps_total"] / (64.0 * max(1, s["wave_iters"])), 4)
            s["steps_per_point"] = round(s["steps_total"] / max(1, s["nvol"] + s["nbdy"]), 3)
            res["variants"][v] = s
            print(f"[{name}] {v:6s} " + " ".join(f"{k[3:]} {s[k]:.3f}" for k in TIMES) +
                  f" steps/pt {s['steps_per_point']} stepmax {s['stepmax']} lockstep {s['lockstep_efficiency']}"
                  f" src {s['nvol_src']}/{s['nbdy_src']}", flush=True)

        # the last round's outputs: class (i) points must agree with the plain call's
        vol_walk = np.nonzero(((hit & 15) == 1) & (pc == 1))[0]
        mb = min_bary(bg, new.xyz, elem, vol_walk)
        ci = vol_walk[mb > EPS]
        res["class_i_points"] = int(ci.size)
        base = dict(el=out["plain"]["el"].download(), hit=out["plain"]["hit"].download())
        assert np.array_equal(base["el"], elem), "the plain call is not reproducible"
        res["agreement"] = {}
        for v in ("near", "stale"):
            el, ht = out[v]["el"].download(), out[v]["hit"].download()
            a = {"elem_differs": int((el != base["el"]).sum()), "hit_differs": int((ht != base["hit"]).sum()),
                 "class_i_elem_differs": int((el[ci] != base["el"][ci]).sum()), "class_i_row_differs": 0}
            for x, y in zip([out["plain"]["mo"]] + out["plain"]["fo"], [out[v]["mo"]] + out[v]["fo"]):
                p, m = x.download(), y.download()
                a["class_i_row_differs"] += int((p[ci].view(np.uint64) != m[ci].view(np.uint64)).any(axis=1).sum())
                del p, m
            res["agreement"][v] = a
            print(f"[{name}] {v}: {a}", flush=True)
            if a["class_i_elem_differs"] or a["class_i_row_differs"]:
                raise SystemExit(f"{name}/{v}: class (i) points differ from the plain call")
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--configs", default="cfg3,cfg4")
    ap.add_argument("--rounds", type=int, default=9)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out", default=os.path.join(ROOT, "bench_out", "point_map", "point_map.json"))
    a = ap.parse_args()
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    res = {"what": "plain (seed grids) vs mapped (pmmg_hip_set_point_map) calls alternating on one context, device "
                   "mode, tet8 records, one array per solution; medians over the rounds",
           "results": []}
    for name in a.configs.split(","):
        res["results"].append(run_config(name, a.rounds, a.warmup))
        with open(a.out, "w") as f:  # (written after every config)
            json.dump(res, f, indent=1)
            f.write("\n")
    print("RESULT " + json.dumps(res), flush=True)


if __name__ == "__main__":
    main()
