"""Times of pmmg_hip_metis_graph (the METIS element graph of a group and its
metric weights) on the adapted mesh of a config, against the
route a caller had before it: pmmg_hip_compute_wgt_faces over the list of all
interior faces, then truncation and compaction on the host.

  python3 tools/metis_graph_time.py --config cfg4 --out bench_out/graph/cfg4.json

The adapted mesh is the config's new lattice with its connectivity and its
adjacency, the metric the config's analytic metric at the new points, as in
tools/mesh_stats_time.py; the numberings are that tool's (`lattice`: the
generator's order, `mmg`: synth.mmg_like_perm on the vertices).

Every call is synchronous and bracketed by two HIP events on the null stream
(tools/mesh_stats_time.py); one warm-up (allocates the scratch), then
--rounds timed calls, medians with min / max.  Per numbering:
  graph_wgt / graph_nowgt    pmmg_hip_metis_graph with and without weights
                             (tetv + adja input, outputs of 4 ne rows)
  faces_kernel               pmmg_hip_compute_wgt_faces over the full
                             interior-face list: the device part of the old
                             route alone
  faces_upload_ms            the face list's upload (8 B per face), wall clock
  host_compact_ms            max((int)w, 1), the row counts and their prefix
                             sum with numpy on the downloaded doubles, wall
                             clock (the download itself: faces_download_ms)
and the algorithmic bytes ne (32 + 4 + 32) + np (24 + 8 met_size) of the
weighted call (tetra row and links, xadj, 4 entries of both lists; vertex
rows once), ne (16 + 4 + 16) of the unweighted one, as a fraction of 8 TB/s.
The fused weights are compared with the old route's, entry by entry."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

from mesh_stats_time import Events  # noqa: E402
from parmmg_amd import configs, synth  # noqa: E402
from parmmg_amd.transfer import TransferContext  # noqa: E402

HBM_PEAK = 8.0e12  # B/s


def face_list(adja, chunk=1 << 23):
    """(tetra, face) of every non-zero link in (tetra, face) order, int32 [n, 2]"""
    parts = []
    for k0 in range(0, adja.shape[0], chunk):
        k, f = np.nonzero(adja[k0:k0 + chunk])
        parts.append(np.stack([(k + k0 + 1).astype(np.int32), f.astype(np.int32)], axis=1))
    return np.ascontiguousarray(np.concatenate(parts))


def stats(v):
    return {"median": round(float(np.median(v)), 4), "min": round(min(v), 4), "max": round(max(v), 4)}


def run(name, rounds, numberings):
    w = configs.SHORT[name]
    t0 = time.time()
    new = synth.lattice(w.kind, w.n_new, jitter=w.jitter_new, seed=synth.SEED, with_trias=False)
    met0 = synth.solution(w.metric, new.xyz)
    ne, npt, ms_ = int(new.ne), int(new.np), int(met0.shape[1])
    faces = face_list(new.adja)
    print(f"[{name}] adapted mesh in {time.time() - t0:.1f} s: {ne} tetra, {npt} vertices, met_size {ms_}, "
          f"{faces.shape[0]} graph entries", flush=True)
    bytes_w = ne * (32 + 4 + 32) + npt * (24 + 8 * ms_)
    bytes_u = ne * (16 + 4 + 16)
    res = {"config": w.name, "ne": ne, "np": npt, "met_size": ms_, "nadjncy": int(faces.shape[0]), "rounds": rounds,
           "bytes_weighted": bytes_w, "bytes_unweighted": bytes_u, "numberings": {}}
    for numbering in numberings:
        xyz, met, tetv = new.xyz, met0, new.tetv
        if numbering == "mmg":
            perm = synth.mmg_like_perm(npt)
            inv = np.empty(npt, np.int32)
            inv[perm] = np.arange(1, npt + 1, dtype=np.int32)
            xyz, met = np.ascontiguousarray(xyz[perm]), np.ascontiguousarray(met[perm])
            tetv = np.ascontiguousarray(inv[tetv - 1])
        with TransferContext(0) as ctx:
            ev = Events()
            dx, dt, da, dm = ctx.upload(xyz), ctx.upload(tetv), ctx.upload(new.adja), ctx.upload(met)
            out = (ctx.empty((ne + 1,), np.int32), ctx.empty((4 * ne,), np.int32), ctx.empty((4 * ne,), np.int32))
            t1 = time.perf_counter()
            df = ctx.upload(faces)
            up_ms = 1e3 * (time.perf_counter() - t1)
            dw = ctx.empty((faces.shape[0],), np.float64)
            calls = {"graph_wgt": lambda: ctx.metis_graph(dx, dt, adja=da, met=dm, out=out),
                     "graph_nowgt": lambda: ctx.metis_graph(None, dt, adja=da, weights=False, out=out),
                     "faces_kernel": lambda: ctx.compute_wgt_faces(dx, dt, df, dm, dw)}
            ms = {k: [] for k in calls}
            for k, fn in calls.items():
                _, t, _ = ev.time(fn)
                print(f"[{name}] {numbering} warm-up {k}: {t:.3f} ms", flush=True)
            for _ in range(rounds):
                for k, fn in calls.items():
                    ms[k].append(ev.time(fn)[1])
            # the old route's host side, and the comparison of the two routes' weights
            calls["graph_wgt"]()
            n = faces.shape[0]
            t1 = time.perf_counter()
            wd = dw.download()
            down_ms = 1e3 * (time.perf_counter() - t1)
            t1 = time.perf_counter()
            wi = np.maximum(wd.astype(np.int32), 1)
            xadj = np.zeros(ne + 1, np.int32)
            np.cumsum(np.count_nonzero(new.adja, axis=1), out=xadj[1:])
            compact_ms = 1e3 * (time.perf_counter() - t1)
            got_x = out[0].download()
            got_w = out[2].download()[:n]
            same = bool((got_w == wi).all() and (got_x == xadj).all())
            for d in (dx, dt, da, dm, df, dw) + out:
                d.free()
        m = {k: stats(v) for k, v in ms.items()}
        m.update(faces_upload_ms=round(up_ms, 2), faces_download_ms=round(down_ms, 2),
                 host_compact_ms=round(compact_ms, 2), same_as_old_route=same,
                 weighted_fraction_of_hbm_peak=round(bytes_w / (1e-3 * m["graph_wgt"]["median"]) / HBM_PEAK, 4),
                 unweighted_fraction_of_hbm_peak=round(bytes_u / (1e-3 * m["graph_nowgt"]["median"]) / HBM_PEAK, 4),
                 weighted_GBps=round(bytes_w / (1e6 * m["graph_wgt"]["median"]), 1),
                 unweighted_GBps=round(bytes_u / (1e6 * m["graph_nowgt"]["median"]), 1))
        res["numberings"][numbering] = m
        print(f"[{name}] {numbering}: " + json.dumps(m), flush=True)
        if not same:
            raise SystemExit("the fused weights differ from the old route's")
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--config", default="cfg4")
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--numberings", default="lattice,mmg")
    ap.add_argument("--out", default=os.path.join(ROOT, "bench_out", "graph", "metis_graph.json"))
    a = ap.parse_args()
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    res = run(a.config, a.rounds, a.numberings.split(","))
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print("RESULT " + json.dumps(res), flush=True)


if __name__ == "__main__":
    main()
