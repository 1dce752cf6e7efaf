"""Times of the adapted mesh's reports on the device: pmmg_hip_tetra_qual,
pmmg_hip_qual_histo and pmmg_hip_edge_lengths (without lists) on the adapted
mesh of a config, device arrays, one live context per edge-table hash:

  python3 tools/gpu_job.py --tag r08a "py tools/mesh_stats_time.py --config cfg4 --out bench_out/r08a/mesh_stats.json"

The adapted mesh is the config's new lattice with its connectivity
(synth.lattice(kind, n_new, jitter)); its metric is the config's analytic
metric evaluated at the new points (what the transfer interpolates, without
running the transfer here: the reports only read the rows).  --numbering
renumbers its vertices: `lattice` keeps the generator's (spatially coherent)
order, `mmg` is synth.mmg_like_perm (one point in six moved to the end, as
after an adaptation), `shuffled` a random permutation; the tetra keep their
order.

The three calls are synchronous, so each is bracketed by two HIP events
recorded on the null stream (the first completes at once, the second after
the call has returned): the event time is the call as its caller sees it —
kernels, the table's memsets, the read-back of the result — and the wall
clock beside it shows the same thing.  One warm-up call each (allocates the
scratch), then --rounds timed calls; medians.

Written per hash mode (PMMG_HIP_EDGEHASH 0: a mix of the whole key, 1: a run
of slots per low vertex): the three times, nedge, the scratch and table
bytes, and the algorithmic GB/s of qual_histo at 12 B per tetra (the first
vertex id, 4 B, and the quality, 8 B; the kernel loads the whole 16 B row:
24 B per tetra)."""
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
from parmmg_amd.transfer import TransferContext  # noqa: E402

SLAB_BYTES = 16384 * 32 + 34 * 8 + 512  # the per-block slab, the counters, the result record


class Events:
    """two HIP events on the null stream around a synchronous call"""

    def __init__(self):
        self.hip = ctypes.CDLL("libamdhip64.so")
        self.a, self.b = ctypes.c_void_p(), ctypes.c_void_p()
        for e in (self.a, self.b):
            if self.hip.hipEventCreate(ctypes.byref(e)) != 0:
                raise RuntimeError("hipEventCreate failed")

    def time(self, fn):
        t0 = time.perf_counter()
        self.hip.hipEventRecord(self.a, None)
        r = fn()
        self.hip.hipEventRecord(self.b, None)
        self.hip.hipEventSynchronize(self.b)
        wall = 1e3 * (time.perf_counter() - t0)
        ms = ctypes.c_float(0.0)
        if self.hip.hipEventElapsedTime(ctypes.byref(ms), self.a, self.b) != 0:
            raise RuntimeError("hipEventElapsedTime failed")
        return r, float(ms.value), wall


def run(name, rounds, numbering):
    w = configs.SHORT[name]
    t0 = time.time()
    new = synth.lattice(w.kind, w.n_new, jitter=w.jitter_new, seed=synth.SEED, with_trias=False)
    met = synth.solution(w.metric, new.xyz)
    if numbering != "lattice":
        perm = synth.mmg_like_perm(new.np) if numbering == "mmg" else np.random.default_rng(7).permutation(new.np)
        inv = np.empty(new.np, np.int32)
        inv[perm] = np.arange(1, new.np + 1, dtype=np.int32)
        new.xyz, met = np.ascontiguousarray(new.xyz[perm]), np.ascontiguousarray(met[perm])
        new.tetv = np.ascontiguousarray(inv[new.tetv - 1])
    print(f"[{name}] adapted mesh in {time.time() - t0:.1f} s: {new.ne} tetra, {new.np} vertices, "
          f"met_size {met.shape[1]}", flush=True)
    res = {"config": w.name, "mesh": "adapted (new) lattice with its connectivity, analytic metric at its points",
           "numbering": numbering, "ne": int(new.ne), "np": int(new.np), "met_size": int(met.shape[1]), "rounds": rounds, "modes": {}}
    for mode in (0, 1):
        os.environ["PMMG_HIP_EDGEHASH"] = str(mode)
        with TransferContext(0) as ctx:
            ev = Events()
            xyz, tetv, dm = ctx.upload(new.xyz), ctx.upload(new.tetv), ctx.upload(met)
            qual = ctx.empty((new.ne,), np.float64)
            qmet = dm if met.shape[1] == 6 else None
            calls = {"tetra_qual": lambda: ctx.tetra_qual(xyz, tetv, qmet, qual)[1],
                     "qual_histo": lambda: ctx.qual_histo(tetv, qual),
                     "edge_lengths": lambda: ctx.edge_lengths(xyz, tetv, dm)}
            out, ms, wall = {}, {k: [] for k in calls}, {k: [] for k in calls}
            for k, fn in calls.items():  # warm-up: allocates the scratch
                out[k], t, _ = ev.time(fn)
                print(f"[{name}] mode {mode} warm-up {k}: {t:.3f} ms", flush=True)
            for _ in range(rounds):
                for k, fn in calls.items():
                    r, t, tw = ev.time(fn)
                    if r != out[k]:
                        raise SystemExit(f"{k}: two calls on the same inputs differ")
                    ms[k].append(t)
                    wall[k].append(tw)
            scratch = ctx.mesh_stats_bytes()
            el = out["edge_lengths"]
            m = {"ms": {k: round(float(np.median(v)), 4) for k, v in ms.items()},
                 "ms_min_max": {k: [round(min(v), 4), round(max(v), 4)] for k, v in ms.items()},
                 "wall_ms": {k: round(float(np.median(v)), 4) for k, v in wall.items()},
                 "nedge": el["nedge"], "ned": el["ned"], "nnull": el["nnull"], "hl": el["hl"],
                 "lmin": el["lmin"], "lmax": el["lmax"], "avlen": el["avlen_sum"] / max(1, el["ned"]),
                 "share_0.71_1.41": round(sum(el["hl"][3:6]) / max(1, el["ned"]), 4),
                 "scratch_bytes": scratch, "table_bytes": scratch - int(new.ne) - SLAB_BYTES,
                 "qual_histo": {k: out["qual_histo"][k] for k in ("ne_used", "min", "max", "iel", "good", "med", "his")},
                 "qual_histo_GBps_at_12B": round(12.0 * new.ne / (1e6 * float(np.median(ms["qual_histo"]))), 1)}
            res["modes"][str(mode)] = m
            print(f"[{name}] mode {mode}: " + " ".join(f"{k} {v:.3f} ms" for k, v in m["ms"].items()) +
                  f" nedge {m['nedge']} table {m['table_bytes'] / 1e9:.2f} GB qual_histo {m['qual_histo_GBps_at_12B']} GB/s",
                  flush=True)
    a, b = res["modes"]["0"], res["modes"]["1"]
    for k in ("nedge", "ned", "nnull", "hl", "lmin", "lmax", "avlen"):
        if a[k] != b[k]:
            raise SystemExit(f"the two hash modes differ in {k}")
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--config", default="cfg4")
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "bench_out", "mesh_stats", "mesh_stats.json"))
    ap.add_argument("--numbering", default="lattice", choices=["lattice", "mmg", "shuffled"])
    a = ap.parse_args()
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    res = run(a.config, a.rounds, a.numbering)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print("RESULT " + json.dumps(res), flush=True)


if __name__ == "__main__":
    main()
