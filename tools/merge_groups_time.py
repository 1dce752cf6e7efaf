"""Times of pmmg_hip_merge_groups (the groups of a rank joined into one mesh,
DESIGN.md §14) beside pmmg_hip_split_groups, its inverse, on the adapted mesh
of a config.

  python3 tools/merge_groups_time.py --config cfg4 --out bench_out/merge/cfg4.json

The adapted mesh, its two tetra numberings (`lattice`, `mmg`) and its two
partitions (`slabs`: 16 slabs along x; `islands`: the slabs with cubes
recoloured) are those of tools/contiguity_time.py and
tools/split_groups_time.py.

Every call is synchronous and bracketed by two HIP events on the null stream;
one warm-up (allocates the scratch), then --rounds timed calls, medians with
min / max.  Per numbering and partition, from the same process:
  split     pmmg_hip_split_groups with old_tet and tet8_out, the lists sized
            by a call with caps of 0 beforehand (not timed)
  merge     pmmg_hip_merge_groups on that split's outputs (tet8 rows, the four
            lists, colours), every output written: new_pt, new_tet, src_pt,
            src_tet, tetv_out, mark_out, node_val, face_val
  gather    pmmg_hip_gather_rows of xyz (3) and of a 6-double metric through
            src_pt, and pmmg_hip_gather_rows_i32 of one int through src_tet

Bytes of the merge: a single read of the inputs (16 per tetra of vertex ids, 8
per node entry, 8 per face entry) plus a single write of the outputs (28 per
tetra of new_tet + src_tet + tetv_out + mark_out, 4 per input point of new_pt,
4 per merged point of src_pt, 4 per node and per face position).  Their
quotient by the median time, as a fraction of 8 TB/s, is what the call as a
whole reaches: its launches, its two read-backs, the memsets of its scratch
and the passes' own traffic are all inside the time."""
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
    color = np.ascontiguousarray(np.arange(NSLAB), np.int32)
    for numbering in numberings:
        adja, tetv, parts = new.adja, new.tetv, {"slabs": slab0, "islands": isl0}
        if numbering == "mmg":
            perm = synth.mmg_like_perm(ne)
            adja, tetv = renumbered(new.adja, perm), np.ascontiguousarray(new.tetv[perm])
            parts = {k: np.ascontiguousarray(v[perm]) for k, v in parts.items()}
        m = {}
        with TransferContext(0) as ctx:
            ev = Events()
            da, dt = ctx.upload(adja), ctx.upload(tetv)
            old_tet, tet8 = ctx.empty((ne,), np.int32), ctx.empty((ne, 8), np.int32)
            for pname, part in parts.items():
                dp = ctx.upload(part)
                count = (_native.HipSplitCount * NSLAB)()
                nn, nf = ctypes.c_int(0), ctypes.c_int(0)

                def split(caps, lists):
                    return ctx.lib.pmmg_hip_split_groups(
                        ctx.h, npv, ne, _p(dt), _p(da), None, _p(dp), NSLAB, None, None, 0, 0, count, caps[0], caps[1],
                        caps[2], _p(old_tet), None, None, None, _p(tet8), *[_p(a) for a in lists], ctypes.byref(nn),
                        ctypes.byref(nf))

                split((0, 0, 0), [None] * 5)  # sizes the lists (and is the warm-up: the scratch is allocated)
                tot = [sum(getattr(c, k) for c in count) for k in ("ne", "np", "nface", "nnode")]
                if tot[0] != ne:
                    raise RuntimeError("split_groups: " + ctx.error())
                lists = [ctx.empty((tot[1],), np.int32)] + [ctx.empty((tot[2],), np.int32) for _ in range(2)]
                lists += [ctx.empty((tot[3],), np.int32) for _ in range(2)]
                ms = []
                for i in range(rounds + 1):
                    ok, t, _ = ev.time(lambda: split(tot[1:], lists))
                    if not ok:
                        raise RuntimeError("split_groups: " + ctx.error())
                    if i:
                        ms.append(t)
                e = dict(split=stats(ms), points=tot[1], face_entries=tot[2], node_entries=tot[3],
                         node_positions=nn.value, face_positions=nf.value)
                # the merge of these groups
                out = dict(new_pt=ctx.empty((tot[1],), np.int32), new_tet=ctx.empty((ne,), np.int32),
                           src_pt=ctx.empty((tot[1],), np.int32), src_tet=ctx.empty((ne,), np.int32),
                           tetv_out=ctx.empty((ne, 4), np.int32), mark_out=ctx.empty((ne,), np.int32),
                           node_val=ctx.empty((nn.value,), np.int32), face_val=ctx.empty((nf.value,), np.int32))
                npo, neo = ctypes.c_int(0), ctypes.c_int(0)

                def merge():
                    return ctx.lib.pmmg_hip_merge_groups(
                        ctx.h, NSLAB, count, None, _p(tet8), _p(lists[3]), _p(lists[4]), _p(lists[1]), _p(lists[2]),
                        nn.value, nf.value, _p(color), tot[1], _p(out["new_pt"]), _p(out["new_tet"]), _p(out["src_pt"]),
                        _p(out["src_tet"]), _p(out["tetv_out"]), _p(out["mark_out"]), _p(out["node_val"]),
                        _p(out["face_val"]), ctypes.byref(npo), ctypes.byref(neo))

                ms = []
                for i in range(rounds + 1):
                    ok, t, _ = ev.time(merge)
                    if not ok:
                        raise RuntimeError("merge_groups: " + ctx.error())
                    if i:
                        ms.append(t)
                if (npo.value, neo.value) != (npv, ne):
                    raise RuntimeError(f"merge_groups: {npo.value} points, {neo.value} tetra of {npv}, {ne}")
                nbytes = ne * 16 + 8 * tot[2] + 8 * tot[3] + ne * 28 + 4 * tot[1] + 4 * npv + 4 * (nn.value + nf.value)
                e.update(merge=stats(ms), merged_points=npo.value, merge_bytes=nbytes)
                e["merge_fraction_of_hbm_peak"] = round(nbytes / (1e-3 * e["merge"]["median"]) / HBM_PEAK, 4)
                e["merge_over_split"] = round(e["merge"]["median"] / e["split"]["median"], 3)
                # the rows of the merged mesh through the maps
                dxyz = ctx.upload(np.zeros((tot[1], 3)))
                dmet = ctx.upload(np.zeros((tot[1], 6)))
                gx, gm = ctx.empty((npv, 3), np.float64), ctx.empty((npv, 6), np.float64)
                src_pt = out["src_pt"]
                src_pt.shape, src_pt.nbytes = (npv,), 4 * npv
                dref, gref = ctx.upload(np.zeros(ne, np.int32)), ctx.empty((ne,), np.int32)

                def gather():
                    ctx.gather_rows(src_pt, dxyz, out=gx)
                    ctx.gather_rows(src_pt, dmet, out=gm)
                    ctx.gather_rows_i32(out["src_tet"], dref, out=gref)

                ev.time(gather)
                e["gather_xyz_met6_ref"] = stats([ev.time(gather)[1] for _ in range(rounds)])
                for d in lists + list(out.values()) + [dp, dxyz, dmet, gx, gm, dref, gref]:
                    d.free()
                m[pname] = e
                print(f"[{name}] {numbering} {pname}: " + json.dumps(e), flush=True)
            for d in (da, dt, old_tet, tet8):
                d.free()
        res["numberings"][numbering] = m
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--config", default="cfg4")
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--islands", type=int, default=300)
    ap.add_argument("--numberings", default="lattice,mmg")
    ap.add_argument("--out", default=os.path.join(ROOT, "bench_out", "merge", "merge_groups.json"))
    a = ap.parse_args()
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    res = run(a.config, a.rounds, a.numberings.split(","), a.islands)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print("RESULT " + json.dumps(res), flush=True)


if __name__ == "__main__":
    main()
