"""Times of pmmg_hip_part_subgroups and pmmg_hip_fix_contiguity (the subgroups
of a partition and their fix) on the adapted mesh of a config.

  python3 tools/contiguity_time.py --config cfg4 --out bench_out/contig/cfg4.json

The adapted mesh is the config's new lattice with its adjacency, as in
tools/metis_graph_time.py.  Only the adjacency and the colours are read, so the
numbering that matters is the tetra's: `lattice` is the generator's order,
`mmg` moves one tetra in six to the end (synth.mmg_like_perm on the tetra, the
links renumbered), as Mmg appends the elements it creates.

Partitions, from the centroid u normalised to the bounding box:
  one      part == NULL, the group check
  slabs    16 slabs along x
  islands  the slabs, then --islands cubes of a 64^3 grid of the box recoloured
           (side 1 to 4 cells, random colour): the fix has work to do

Every call is synchronous and bracketed by two HIP events on the null stream
(tools/mesh_stats_time.py); one warm-up (allocates the scratch), then --rounds
timed calls, medians with min / max.  Per numbering and partition:
  subgroups        pmmg_hip_part_subgroups with head and flag, its subgroup
                   count, hooking rounds and flatten passes
  fix              pmmg_hip_fix_contiguity on a fresh copy of the colours (the
                   copy is outside the events), its counts and passes
and per numbering the unweighted pmmg_hip_metis_graph call, which reads the
same link rows, as the yardstick.  Bytes of a hooking round: ne (16 link row +
4 colour + 4 label), the neighbours' colours and labels (up to 4 x 8 more,
gathered) not counted; of a flatten pass: ne x 8 at the least.  Both as a
fraction of 8 TB/s at the round's / pass's average time are upper bounds of
what the kernels reach: the calls' time includes the read-backs between
launches."""
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
NSLAB = 16
GRID = 64


def stats(v):
    return {"median": round(float(np.median(v)), 4), "min": round(min(v), 4), "max": round(max(v), 4)}


def colours(new, nisland):
    """(slabs, islands) int32 [ne] of the mesh in the generator's order"""
    lo, hi = new.xyz.min(axis=0), new.xyz.max(axis=0)
    cell = np.zeros(new.ne, np.int64)
    slab = None
    for ax in range(3):  # (axis by axis: a [ne, 3] centroid array of a 100M-tetra mesh is 3 GB)
        u = (new.xyz[:, ax][new.tetv - 1].mean(axis=1) - lo[ax]) / (hi[ax] - lo[ax])
        if ax == 0:
            slab = np.minimum((u * NSLAB).astype(np.int32), NSLAB - 1)
        cell = cell * GRID + np.minimum((u * GRID).astype(np.int64), GRID - 1)
    rng = np.random.default_rng(5)
    paint = np.full((GRID, GRID, GRID), -1, np.int32)
    for _ in range(nisland):
        c = rng.integers(0, GRID, 3)
        s = rng.integers(1, 5)
        paint[c[0]:c[0] + s, c[1]:c[1] + s, c[2]:c[2] + s] = rng.integers(0, NSLAB)
    p = paint.reshape(-1)[cell]
    return slab, np.where(p >= 0, p, slab).astype(np.int32)


def renumbered(adja, perm):
    """adja of the mesh with new tetra i = old tetra perm[i]"""
    inv = np.empty(perm.size, np.int32)
    inv[perm] = np.arange(1, perm.size + 1, dtype=np.int32)
    a = adja[perm]
    nz = a != 0
    out = np.zeros_like(a)
    out[nz] = 4 * inv[a[nz] // 4 - 1] + a[nz] % 4
    return np.ascontiguousarray(out)


def run(name, rounds, numberings, nisland):
    w = configs.SHORT[name]
    t0 = time.time()
    new = synth.lattice(w.kind, w.n_new, jitter=w.jitter_new, seed=synth.SEED, with_trias=False)
    ne = int(new.ne)
    slab0, isl0 = colours(new, nisland)
    print(f"[{name}] adapted mesh and colours in {time.time() - t0:.1f} s: {ne} tetra", flush=True)
    res = {"config": w.name, "ne": ne, "rounds": rounds, "islands": nisland, "bytes_hook_round": ne * 24,
           "bytes_flatten_pass": ne * 8, "numberings": {}}
    for numbering in numberings:
        adja, tetv, parts = new.adja, new.tetv, {"one": None, "slabs": slab0, "islands": isl0}
        if numbering == "mmg":
            perm = synth.mmg_like_perm(ne)
            adja, tetv = renumbered(new.adja, perm), np.ascontiguousarray(new.tetv[perm])
            parts = {k: (None if v is None else np.ascontiguousarray(v[perm])) for k, v in parts.items()}
        m = {}
        with TransferContext(0) as ctx:
            ev = Events()
            da, dt = ctx.upload(adja), ctx.upload(tetv)
            head, flag, work = (ctx.empty((ne,), np.int32) for _ in range(3))
            out = (ctx.empty((ne + 1,), np.int32), ctx.empty((4 * ne,), np.int32), None)
            graph = lambda: ctx.metis_graph(None, dt, adja=da, weights=False, out=out)
            ev.time(graph)
            m["graph_nowgt"] = stats([ev.time(graph)[1] for _ in range(rounds)])
            for pname, part in parts.items():
                dp = None if part is None else ctx.upload(part)
                ncolor = 1 if part is None else NSLAB
                sub = lambda: ctx.part_subgroups(None, adja=da, part=dp, ncolor=ncolor, head=head, flag=flag,
                                                 cap=1 << 14)
                r, t, _ = ev.time(sub)
                print(f"[{name}] {numbering} {pname} warm-up subgroups: {t:.3f} ms, {r['sub'].shape[0]} subgroups, "
                      f"{r['rounds']} rounds, {r['passes']} passes", flush=True)
                ms = [ev.time(sub)[1] for _ in range(rounds)]
                e = {"subgroups": stats(ms), "nsub": int(r["sub"].shape[0]), "ncomp_max": int(r["ncomp"].max()),
                     "hook_rounds": r["rounds"], "flatten_passes": r["passes"]}
                per = 1e-3 * e["subgroups"]["median"] / (r["rounds"] + r["passes"])
                e["launch_avg_ms"] = round(1e3 * per, 4)
                e["hook_round_fraction_of_hbm_peak_at_avg"] = round(ne * 24 / per / HBM_PEAK, 4)
                if part is not None:
                    fms, fr = [], None
                    for i in range(rounds + 1):
                        ctx.lib.pmmg_hip_memcpy_h2d(ctx.h, work.ptr, part.ctypes.data, part.nbytes)
                        fr, t, _ = ev.time(lambda: ctx.fix_contiguity(None, work, ncolor, adja=da))
                        if i:
                            fms.append(t)
                    after = ctx.part_subgroups(None, adja=da, part=work, ncolor=ncolor, cap=1 << 14)
                    e.update(fix=stats(fms), fix_counts=fr, ncomp_max_after=int(after["ncomp"].max()))
                    dp.free()
                m[pname] = e
                print(f"[{name}] {numbering} {pname}: " + json.dumps(e), flush=True)
            for d in (da, dt, head, flag, work, out[0], out[1]):
                d.free()
        res["numberings"][numbering] = m
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--config", default="cfg4")
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--islands", type=int, default=300)
    ap.add_argument("--numberings", default="lattice,mmg")
    ap.add_argument("--out", default=os.path.join(ROOT, "bench_out", "contig", "contiguity.json"))
    a = ap.parse_args()
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    res = run(a.config, a.rounds, a.numberings.split(","), a.islands)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print("RESULT " + json.dumps(res), flush=True)


if __name__ == "__main__":
    main()
