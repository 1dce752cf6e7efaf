"""Times of the exhaustive searches on the workload of
tests/test_gpu_fallback_scale.py (1.05M tetra; 2400 volume and 2300 surface
queries, every walk stopped after one step by PMMG_HIP_MAXSTEP=1), over
repeated calls on one context:

  python3 tools/fallback_time.py --rounds 20 --out bench_out/fallback.json

ms_fallback is the main stream from the volume kernel's end to the end of the
volume queries' closest search, ms_bdy the surface branch with its searches
(pmmg_hip_stats).  One warm-up call (buffers sized, kernels loaded), then
--rounds timed ones: medians with min / max, and the counters of the last."""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(1, os.path.join(ROOT, "tests"))

os.environ["PMMG_HIP_MAXSTEP"] = "1"  # read when the context is created

import test_gpu_fallback_scale as scale  # noqa: E402
from parmmg_amd import synth  # noqa: E402
from parmmg_amd.transfer import TransferContext, pack_tet8  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=20)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    bg = synth.lattice(synth.CUBE, scale.N_OLD)
    met = synth.solution(synth.F_ANI, bg.xyz)
    fields = [synth.solution(synth.F_SCALAR, bg.xyz), synth.solution(synth.F_VECTOR, bg.xyz)]
    xyz, pc = scale._queries(np.random.default_rng(2025), n_in=2000, n_out=400, n_face=2000, n_far=300)
    n = xyz.shape[0]
    ctx = TransferContext(0, sort=False)
    d = [ctx.upload(x) for x in (bg.xyz, pack_tet8(bg.tetv, bg.adja), bg.triv, bg.adjt)]
    ctx.set_background_tet8(*d, scale.HAUSD)
    ctx.set_solutions(ctx.upload(met), [ctx.upload(f) for f in fields])
    q, c = ctx.upload(xyz), ctx.upload(pc)
    mo = ctx.empty((n, 6), np.float64)
    fo = [ctx.empty((n, f.shape[1]), np.float64) for f in fields]
    el, hit = ctx.empty((n,), np.int32), ctx.empty((n,), np.int8)
    times = {"ms_fallback": [], "ms_bdy": [], "ms_total": []}
    for r in range(a.rounds + 1):
        s = ctx.locate_interp(q, c, mo, fo, el, hit).as_dict()
        if r:
            for k in times:
                times[k].append(s[k])
    ctx.close()
    res = {k: {"median": round(float(np.median(v)), 4), "min": round(min(v), 4), "max": round(max(v), 4)}
           for k, v in times.items()}
    res["counters"] = {k: s[k] for k in ("nvol_exhaust", "nvol_closest", "nbdy_exhaust", "nbdy_closest", "nbdy_stale")}
    res["rounds"] = a.rounds
    res["so"] = os.path.basename(os.environ.get("PMMG_HIP_SO", "libpmmg_hip.so"))
    print(json.dumps(res), flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
