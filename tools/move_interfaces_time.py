"""Times of pmmg_hip_ifc_seed and pmmg_hip_ifc_layers (the interface
displacement) on the adapted mesh of a config.

  python3 tools/move_interfaces_time.py --config cfg4 --out bench_out/moveifc/cfg4.json

The adapted mesh, its two tetra numberings (`lattice`, `mmg`) and its two
partitions (`slabs`: 16 slabs along x; `islands`: the slabs with cubes
recoloured) are those of tools/contiguity_time.py.  The weight of a colour is
its tetra count plus its index (all distinct); every colour is given as not
local (nelem = -1), so no layer is blocked and the brake's host decision is a
loop over 16 zeros.

Every call is synchronous and bracketed by two HIP events on the null stream;
one warm-up round (allocates the scratch), then --rounds timed rounds, medians
with min / max.  A round uploads the marks again (not timed), then times
  seed      pmmg_hip_ifc_seed
  layer l   pmmg_hip_ifc_layers with nlayers = 1 from the state the round's
            earlier calls left, l = 1 .. --layers
and, once per partition from the same process, pmmg_hip_part_subgroups and
pmmg_hip_split_groups (old_tet and tet8_out) on the same colours.

Bytes, a single read of the inputs and a single write of the outputs: the
seed reads 20 per tetra (tetv, mark) and writes 5 per point (colour, flag); a
layer reads 20 per tetra and 5 per point and writes 4 per tetra and 5 per
point.  Their quotient by the median time, as a fraction of 8 TB/s, is what
the call as a whole reaches: its launches, its read-backs, its copies in and
out of the scratch and the passes' own traffic (three passes read the tetra
rows again) are all inside the time."""
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


def run(name, rounds, numberings, nisland, nlayers):
    w = configs.SHORT[name]
    t0 = time.time()
    new = synth.lattice(w.kind, w.n_new, jitter=w.jitter_new, seed=synth.SEED, with_trias=False)
    ne, npv = int(new.ne), int(new.np)
    slab0, isl0 = colours(new, nisland)
    print(f"[{name}] adapted mesh and colours in {time.time() - t0:.1f} s: {ne} tetra, {npv} points", flush=True)
    res = {"config": w.name, "ne": ne, "np": npv, "rounds": rounds, "islands": nisland, "layers": nlayers,
           "numberings": {}}
    none = np.full(NSLAB, -1, np.int32)
    zero = np.zeros(NSLAB, np.int32)
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
            head, flag = ctx.empty((ne,), np.int32), ctx.empty((ne,), np.int32)
            color, front = ctx.empty((npv,), np.int32), ctx.empty((npv,), np.uint8)
            old_tet, tet8 = ctx.empty((ne,), np.int32), ctx.empty((ne, 8), np.int32)
            for pname, part in parts.items():
                part = np.ascontiguousarray(part, np.int32)
                weight = (np.bincount(part, minlength=NSLAB) + np.arange(NSLAB) + 1).astype(np.int32)
                dp = ctx.upload(part)
                seed_ms, layer_ms, moved = [], [[] for _ in range(nlayers)], [0] * nlayers
                done, blocked, mv = ctypes.c_int(0), ctypes.c_int(0), ctypes.c_int(0)
                for r in range(rounds + 1):
                    ctx._ck(ctx.lib.pmmg_hip_memcpy_h2d(ctx.h, _p(dp), _p(part), part.nbytes), "h2d")
                    ok, t, _ = ev.time(lambda: ctx.lib.pmmg_hip_ifc_seed(ctx.h, npv, ne, _p(dt), None, _p(dp), NSLAB,
                                                                         _p(weight), _p(color), _p(front)))
                    if not ok:
                        raise RuntimeError("ifc_seed: " + ctx.error())
                    if r:
                        seed_ms.append(t)
                    for l in range(nlayers):
                        nelem = none.copy()
                        ok, t, _ = ev.time(lambda: ctx.lib.pmmg_hip_ifc_layers(
                            ctx.h, npv, ne, _p(dt), None, _p(dp), NSLAB, _p(weight), _p(nelem), _p(zero), _p(color),
                            _p(front), 0, None, None, 1, ctypes.byref(done), ctypes.byref(blocked), ctypes.byref(mv)))
                        if not ok or done.value != 1:
                            raise RuntimeError("ifc_layers: " + ctx.error())
                        moved[l] = mv.value
                        if r:
                            layer_ms[l].append(t)
                e = {"seed": stats(seed_ms), "layers": [stats(x) for x in layer_ms], "moved": moved}
                sbytes, lbytes = 20 * ne + 5 * npv, 24 * ne + 10 * npv
                e.update(seed_bytes=sbytes, layer_bytes=lbytes, layer_bytes_per_tetra=round(lbytes / ne, 2))
                e["seed_fraction_of_hbm_peak"] = round(sbytes / (1e-3 * e["seed"]["median"]) / HBM_PEAK, 4)
                e["layer_fraction_of_hbm_peak"] = [round(lbytes / (1e-3 * s["median"]) / HBM_PEAK, 4) for s in e["layers"]]
                # beside it, on the same colours (the marks as uploaded)
                ctx._ck(ctx.lib.pmmg_hip_memcpy_h2d(ctx.h, _p(dp), _p(part), part.nbytes), "h2d")
                sub = lambda: ctx.part_subgroups(None, adja=da, part=dp, ncolor=NSLAB, head=head, flag=flag, cap=1 << 14)
                ev.time(sub)
                e["part_subgroups"] = stats([ev.time(sub)[1] for _ in range(rounds)])
                count = (_native.HipSplitCount * NSLAB)()
                nn, nf = ctypes.c_int(0), ctypes.c_int(0)

                def call(caps, lists):
                    return ctx.lib.pmmg_hip_split_groups(
                        ctx.h, npv, ne, _p(dt), _p(da), None, _p(dp), NSLAB, None, None, 0, 0, count, caps[0], caps[1],
                        caps[2], _p(old_tet), None, None, None, _p(tet8), *[_p(a) for a in lists], ctypes.byref(nn),
                        ctypes.byref(nf))

                call((0, 0, 0), [None] * 5)
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
                e["split_groups"] = stats(ms)
                for d in lists + [dp]:
                    d.free()
                m[pname] = e
                print(f"[{name}] {numbering} {pname}: " + json.dumps(e), flush=True)
            for d in (da, dt, head, flag, color, front, old_tet, tet8):
                d.free()
        res["numberings"][numbering] = m
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--config", default="cfg4")
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--layers", type=int, default=2)
    ap.add_argument("--islands", type=int, default=300)
    ap.add_argument("--numberings", default="lattice,mmg")
    ap.add_argument("--out", default=os.path.join(ROOT, "bench_out", "moveifc", "move_interfaces.json"))
    a = ap.parse_args()
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    res = run(a.config, a.rounds, a.numberings.split(","), a.islands, a.layers)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print("RESULT " + json.dumps(res), flush=True)


if __name__ == "__main__":
    main()
