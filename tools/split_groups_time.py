"""Times of pmmg_hip_split_groups and pmmg_hip_gather_rows (the sub-meshes and
interfaces of a partition) on the adapted mesh of a config.

  python3 tools/split_groups_time.py --config cfg4 --out bench_out/split/cfg4.json

The adapted mesh, its two tetra numberings (`lattice`, `mmg`) and its two
partitions (`slabs`: 16 slabs along x; `islands`: the slabs with cubes
recoloured) are those of tools/contiguity_time.py.

Every call is synchronous and bracketed by two HIP events on the null stream;
one warm-up (allocates the scratch), then --rounds timed calls, medians with
min / max.  Per numbering and partition:
  split     pmmg_hip_split_groups with old_tet and tet8_out (no new_tet, no
            separate tetv_out / adja_out), the lists sized by a call with
            caps of 0 beforehand (not timed); its counts and first-use rounds
  gather    pmmg_hip_gather_rows of xyz (3) and of a 6-double metric through
            old_pt, the two calls together
and per numbering, from the same process, the unweighted pmmg_hip_metis_graph
and pmmg_hip_part_subgroups calls, which read the same link rows.

Bytes: a single read of the inputs (32 per tetra of tetv + adja, 4 of part)
plus a single write of the outputs (36 per tetra of old_tet + tet8_out, 4 per
point, 8 per face entry, 8 per node entry); for the gather 4 + 72 read and 72
written per point.  Their quotient by the median time, as a fraction of 8 TB/s,
is what the call as a whole reaches: its launches, the read-backs between
them and the passes' own traffic (every pass reads the mesh again) are all
inside the time."""
import argparse
import ctypes
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

from contiguity_time import HBM_PEAK, NSLAB, colours, renumbered, stats  # noqa: E402
from mesh_stats_time import Events  # noqa: E402
from parmmg_amd import _native, configs, synth  # noqa: E402
from parmmg_amd.transfer import TransferContext, _p  # noqa: E402


def run(name, rounds, numberings, nisland):
    w = configs.SHORT[name]
    t0 = time.time()
    new = synth.lattice(w.kind, w.n_new, jitter=w.jitter_new, seed=synth.SEED, with_trias=False)
    ne, npv = int(new.ne), int(new.np)
    slab0, isl0 = colours(new, nisland)
    met = np.ascontiguousarray(synth.solution(synth.F_ANI, new.xyz))
    print(f"[{name}] adapted mesh and colours in {time.time() - t0:.1f} s: {ne} tetra, {npv} points", flush=True)
    res = {"config": w.name, "ne": ne, "np": npv, "rounds": rounds, "islands": nisland, "numberings": {}}
    for numbering in numberings:
        adja, tetv, parts = new.adja, new.tetv, {"slabs": slab0, "islands": isl0}
        if numbering == "mmg":
            perm = synth.mmg_like_perm(ne)
            adja, tetv = renumbered(new.adja, perm), np.ascontiguousarray(new.tetv[perm])
            parts = {k: np.ascontiguousarray(v[perm]) for k, v in parts.items()}
        m = {}
        with TransferContext(0) as ctx:
            ev = Events()
            da, dt, dxyz, dmet = ctx.upload(adja), ctx.upload(tetv), ctx.upload(new.xyz), ctx.upload(met)
            head, flag = ctx.empty((ne,), np.int32), ctx.empty((ne,), np.int32)
            out = (ctx.empty((ne + 1,), np.int32), ctx.empty((4 * ne,), np.int32), None)
            graph = lambda: ctx.metis_graph(None, dt, adja=da, weights=False, out=out)
            ev.time(graph)
            m["graph_nowgt"] = stats([ev.time(graph)[1] for _ in range(rounds)])
            old_tet, tet8 = ctx.empty((ne,), np.int32), ctx.empty((ne, 8), np.int32)
            for pname, part in parts.items():
                dp = ctx.upload(part)
                sub = lambda: ctx.part_subgroups(None, adja=da, part=dp, ncolor=NSLAB, head=head, flag=flag, cap=1 << 14)
                ev.time(sub)
                e = {"part_subgroups": stats([ev.time(sub)[1] for _ in range(rounds)])}
                count = (_native.HipSplitCount * NSLAB)()
                nn, nf = ctypes.c_int(0), ctypes.c_int(0)

                def call(caps, lists):
                    return ctx.lib.pmmg_hip_split_groups(
                        ctx.h, npv, ne, _p(dt), _p(da), None, _p(dp), NSLAB, None, None, 0, 0, count, caps[0], caps[1],
                        caps[2], _p(old_tet), None, None, None, _p(tet8), *[_p(a) for a in lists], ctypes.byref(nn),
                        ctypes.byref(nf))

                call((0, 0, 0), [None] * 5)  # sizes the lists (and is the warm-up: the scratch is allocated)
                tot = [sum(getattr(c, k) for c in count) for k in ("ne", "np", "nface", "nnode")]
                if tot[0] != ne:
                    raise RuntimeError("split_groups: " + ctx.error())
                lists = [ctx.empty((tot[1],), np.int32)] + [ctx.empty((tot[2],), np.int32) for _ in range(2)]
                lists += [ctx.empty((tot[3],), np.int32) for _ in range(2)]
                ms = []
                for i in range(rounds + 1):
                    ok, t, _ = ev.time(lambda: call(tot[1:], lists))
                    if not ok:
                        raise RuntimeError("split_groups: " + ctx.error())
                    if i:
                        ms.append(t)
                nbytes = ne * (32 + 4) + ne * 36 + 4 * tot[1] + 8 * tot[2] + 8 * tot[3]
                e.update(split=stats(ms), points=tot[1], face_entries=tot[2], node_entries=tot[3],
                         owned_faces=nf.value, first_use_rounds=int(ctx.lib.pmmg_hip_split_rounds(ctx.h)),
                         split_bytes=nbytes)
                e["split_fraction_of_hbm_peak"] = round(nbytes / (1e-3 * e["split"]["median"]) / HBM_PEAK, 4)
                gx, gm = ctx.empty((tot[1], 3), np.float64), ctx.empty((tot[1], 6), np.float64)

                def gather():
                    ctx.gather_rows(lists[0], dxyz, out=gx)
                    ctx.gather_rows(lists[0], dmet, out=gm)

                ev.time(gather)
                e["gather_xyz_met6"] = stats([ev.time(gather)[1] for _ in range(rounds)])
                gbytes = tot[1] * (2 * 4 + 2 * 72)
                e["gather_bytes"] = gbytes
                e["gather_fraction_of_hbm_peak"] = round(gbytes / (1e-3 * e["gather_xyz_met6"]["median"]) / HBM_PEAK, 4)
                for d in lists + [gx, gm, dp]:
                    d.free()
                m[pname] = e
                print(f"[{name}] {numbering} {pname}: " + json.dumps(e), flush=True)
            for d in (da, dt, dxyz, dmet, head, flag, out[0], out[1], old_tet, tet8):
                d.free()
        res["numberings"][numbering] = m
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--config", default="cfg4")
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--islands", type=int, default=300)
    ap.add_argument("--numberings", default="lattice,mmg")
    ap.add_argument("--out", default=os.path.join(ROOT, "bench_out", "split", "split_groups.json"))
    a = ap.parse_args()
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    res = run(a.config, a.rounds, a.numberings.split(","), a.islands)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print("RESULT " + json.dumps(res), flush=True)


if __name__ == "__main__":
    main()
