"""One build (PMMG_HIP_SO) of the mesh services: the refusal texts on a 6-tetra cube, then checksums of every
output on a seeded lattice.  Run once per build in a fresh process; the two listings must be identical."""
import ctypes
import hashlib
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
from parmmg_amd import synth  # noqa: E402
from parmmg_amd.transfer import TransferContext, HipSubgroup  # noqa: E402


def sha(a):
    return hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()[:16]


def P(d, off=0):
    return None if d is None else ctypes.c_void_p(d.ptr + off)


def cube6():
    # Kuhn split: one tetra per order of the axes, vertex id 1 + x + 2 y + 4 z
    import itertools
    tet = []
    for perm in itertools.permutations((1, 2, 4)):
        v, row = 0, [1]
        for a in perm:
            v += a
            row.append(v + 1)
        tet.append(row)
    xyz = np.array([[i & 1, (i >> 1) & 1, (i >> 2) & 1] for i in range(8)], np.float64)
    return xyz, np.array(tet, np.int32)


def refusals():
    xyz, tetv = cube6()
    ne, npt = 6, 8
    with TransferContext(0) as ctx:
        L, h = ctx.lib, ctx.h
        say = lambda name, rc: print(f"{name}: rc={rc} | {ctx.error() if not rc else ''}", flush=True)
        dx, dt = ctx.upload(xyz), ctx.upload(tetv)
        pad = ctx.empty((64,), np.int32)
        da, d8 = ctx.build_adjacency(npt, dt)
        adja = da.download()
        print("cube6 adja", sha(adja), "tet8", sha(d8.download()))
        bad_t = tetv.copy(); bad_t[3, 2] = 99
        dbt = ctx.upload(bad_t)
        # a copy of tetv one int into a larger buffer: a base 4 bytes off a 16-byte line
        big = ctx.empty((ne * 8 + 8,), np.int32)
        big.zero()
        pad.zero()
        out_a, out_8 = ctx.empty((ne, 4), np.int32), ctx.empty((ne, 8), np.int32)
        say("build_adjacency NULL tetv", L.pmmg_hip_build_adjacency(h, npt, ne, None, P(out_a), P(out_8)))
        say("build_adjacency no output", L.pmmg_hip_build_adjacency(h, npt, ne, P(dt), None, None))
        say("build_adjacency misaligned tetv", L.pmmg_hip_build_adjacency(h, npt, ne, P(big, 4), P(out_a), None))
        say("build_adjacency misaligned adja", L.pmmg_hip_build_adjacency(h, npt, ne, P(dt), P(big, 8), None))
        say("build_adjacency bad id", L.pmmg_hip_build_adjacency(h, npt, ne, P(dbt), P(out_a), P(out_8)))
        say("build_adjacency ok", L.pmmg_hip_build_adjacency(h, npt, ne, P(dt), P(out_a), P(out_8)))

        nt = ctypes.c_int(0)
        triv, adjt = ctx.empty((64, 3), np.int32), ctx.empty((64, 3), np.int32)
        bb = lambda *a: L.pmmg_hip_build_boundary(h, npt, ne, *a)
        say("build_boundary NULL arrays", bb(None, None, None, None, 64, ctypes.byref(nt), P(triv), P(adjt)))
        say("build_boundary NULL adja", bb(None, P(dt), None, None, 64, ctypes.byref(nt), P(triv), P(adjt)))
        say("build_boundary NULL tetv", bb(None, None, P(da), None, 64, ctypes.byref(nt), P(triv), P(adjt)))
        say("build_boundary misaligned tetv", bb(None, P(big, 4), P(da), None, 64, ctypes.byref(nt), P(triv), P(adjt)))
        say("build_boundary misaligned adja", bb(None, P(dt), P(big, 8), None, 64, ctypes.byref(nt), P(triv), P(adjt)))
        say("build_boundary misaligned tet8", bb(P(big, 4), None, None, None, 64, ctypes.byref(nt), P(triv), P(adjt)))
        say("build_boundary cap too small", bb(P(d8), None, None, None, 3, ctypes.byref(nt), P(triv), P(adjt)))
        print("   nt", nt.value)
        say("build_boundary cap without triv", bb(P(d8), None, None, None, 3, ctypes.byref(nt), None, None))
        say("build_boundary ok", bb(None, P(dt), P(da), None, 64, ctypes.byref(nt), P(triv), P(adjt)))
        print("   nt", nt.value, sha(triv.download()[:nt.value]), sha(adjt.download()[:nt.value]))

        # meshes that are refused after a kernel looked at them
        a_badlink = adja.copy(); a_badlink[2, 1] = 4 * 7 + 0
        t_unused = tetv.copy(); t_unused[4, 0] = 0  # (its neighbours still link to it)
        a_unused_ok = adja.copy()
        a_unused_ok[a_unused_ok // 4 == 5] = 0      # nobody links to row 5 (1-based), row 5 unused: accepted
        d_badlink, d_tun, d_aok = ctx.upload(a_badlink), ctx.upload(t_unused), ctx.upload(a_unused_ok)
        met = ctx.upload(np.full((npt, 1), 0.5))
        n64 = ctypes.c_int64(0)
        xadj, adjncy, adjwgt = ctx.empty((ne + 1,), np.int32), ctx.empty((64,), np.int32), ctx.empty((64,), np.int32)

        def mg(name, tv, aj, t8, cap=64, np_=npt, x=dx, m=met, ms=1, xa=None, an=None, aw="w"):
            w = P(adjwgt) if aw == "w" else aw
            rc = L.pmmg_hip_metis_graph(h, np_, P(x) if x is not None else None, ne, tv, aj, t8, ms,
                                        P(m) if m is not None else None, cap, ctypes.byref(n64),
                                        xa if xa is not None else P(xadj), an if an is not None else P(adjncy), w)
            say("metis_graph " + name, rc)
            print("   nadjncy", n64.value)
            return rc

        mg("NULL arrays", None, None, None)
        mg("NULL arrays, no weights", None, None, None, aw=None)
        mg("NULL tetv with weights", None, P(da), None)
        mg("NULL tetv, no weights (ok)", None, P(da), None, aw=None)
        mg("misaligned tetv", P(big, 4), P(da), None)
        mg("misaligned adja", P(dt), P(big, 8), None)
        mg("misaligned tet8", None, None, P(big, 4))
        mg("misaligned xadj", P(dt), P(da), None, xa=P(pad, 2))
        mg("bad link", P(dt), P(d_badlink), None)
        mg("bad id", P(dbt), P(da), None)
        mg("link to an unused row", P(d_tun), P(da), None)
        mg("unused row nobody links to (ok)", P(d_tun), P(d_aok), None)
        mg("cap too small", P(dt), P(da), None, cap=5)
        mg("adjacency built, np 0", P(dt), None, None, np_=0, aw=None)
        mg("adjacency built (ok)", P(dt), None, None, aw=None)
        mg("adjacency built, bad id", P(dbt), None, None, aw=None)
        mg("packed (ok)", None, None, P(d8))
        print("   xadj", sha(xadj.download()), "adjncy", sha(adjncy.download()[:n64.value]), "adjwgt",
              sha(adjwgt.download()[:n64.value]))

        part = np.array([0, 1, 0, 1, 0, 1], np.int32)
        p_bad = part.copy(); p_bad[3] = 5
        dp, dpb = ctx.upload(part), ctx.upload(p_bad)
        head, flag = ctx.empty((ne,), np.int32), ctx.empty((ne,), np.int32)
        ncomp = (ctypes.c_int * 4)()
        table = (HipSubgroup * 64)()
        nsub, rounds = ctypes.c_int64(0), ctypes.c_int(0)

        def ps(name, tv, aj, t8, pt=dp, ncolor=2, cap=64, hd=None, ptr_part=None):
            pp = ptr_part if ptr_part is not None else (P(pt) if pt is not None else None)
            rc = L.pmmg_hip_part_subgroups(h, ne, tv, aj, t8, pp, ncolor, hd if hd is not None else P(head), P(flag),
                                           ncomp, cap, table, ctypes.byref(nsub), ctypes.byref(rounds))
            say("part_subgroups " + name, rc)
            print("   nsub", nsub.value, "ncomp", list(ncomp)[:ncolor], "rounds", rounds.value)

        nmoved, nmerged, nstuck = ctypes.c_int64(0), ctypes.c_int(0), ctypes.c_int(0)

        def fx(name, tv, aj, t8, pt=dp, ncolor=2, ptr_part=None, counters=True):
            work = ctx.upload(pt.download()) if pt is not None else None
            pp = ptr_part if ptr_part is not None else (P(work) if work is not None else None)
            rc = L.pmmg_hip_fix_contiguity(h, ne, tv, aj, t8, pp, ncolor, ctypes.byref(nmoved),
                                           ctypes.byref(nmerged) if counters else None, ctypes.byref(nstuck))
            say("fix_contiguity " + name, rc)
            print("   moved", nmoved.value, nmerged.value, nstuck.value, "part",
                  sha(work.download()) if work is not None else None)

        for f in (ps, fx):
            f("NULL arrays", None, None, None)
            f("NULL adja (built, ok)", P(dt), None, None)
            f("NULL adja, bad id", P(dbt), None, None)
            f("NULL tetv (ok)", None, P(da), None)
            f("misaligned tetv", P(big, 4), P(da), None)
            f("misaligned adja", P(dt), P(big, 8), None)
            f("misaligned tet8", None, None, P(big, 4))
            f("misaligned part", P(dt), P(da), None, ptr_part=P(pad, 2))
            f("ncolor 0", P(dt), P(da), None, ncolor=0)
            f("part NULL, ncolor 2", P(dt), P(da), None, pt=None)
            f("part NULL, one colour (ok)", P(dt), P(da), None, pt=None, ncolor=1)
            f("bad link", P(dt), P(d_badlink), None)
            f("bad part", P(dt), P(da), None, pt=dpb)
            f("link to an unused row", P(d_tun), P(da), None)
            f("unused row nobody links to (ok)", P(d_tun), P(d_aok), None)
            f("packed (ok)", None, None, P(d8))
        ps("cap too small", P(dt), P(da), None, cap=1)
        ps("negative cap", P(dt), P(da), None, cap=-1)
        ps("misaligned head", P(dt), P(da), None, hd=P(pad, 2))
        fx("NULL counter", P(dt), P(da), None, counters=False)
        print("   head", sha(head.download()), "flag", sha(flag.download()))


def results():
    new = synth.lattice(synth.CUBE, 23, jitter=0.15, seed=synth.SEED, with_trias=False)
    ne, npt = int(new.ne), int(new.np)
    perm = synth.mmg_like_perm(ne)
    tetv = np.ascontiguousarray(new.tetv[perm])
    met = synth.solution(synth.F_ISO, new.xyz)
    print(f"lattice: ne {ne} np {npt} met {met.shape}")
    with TransferContext(0) as ctx:
        dx, dt, dm = ctx.upload(new.xyz), ctx.upload(tetv), ctx.upload(met)
        da, d8 = ctx.build_adjacency(npt, dt)
        adja = da.download()
        print("build_adjacency", sha(adja), sha(d8.download()))
        for kw in (dict(tet8=d8), dict(tetv=dt, adja=da)):
            triv, adjt = ctx.build_boundary(npt, **kw)
            print("build_boundary", sorted(kw), triv.shape, sha(triv.download()), sha(adjt.download()))
        tref = ctx.upload((np.arange(ne) % 3).astype(np.int32))
        triv, adjt = ctx.build_boundary(npt, tet8=d8, tref=tref)
        print("build_boundary tref", triv.shape, sha(triv.download()), sha(adjt.download()))
        for name, kw in (("separate wgt", dict(tetv=dt, adja=da, met=dm)), ("packed wgt", dict(tetv=None, tet8=d8, met=dm)),
                         ("no metric", dict(tetv=dt, adja=da)), ("nowgt from tetv", dict(tetv=dt, weights=False))):
            tv = kw.pop("tetv")
            x, a, w = ctx.metis_graph(dx, tv, **kw)
            print("metis_graph", name, a.shape, sha(x.download()), sha(a.download()), sha(w.download()) if w is not None else None)
        u = new.xyz[:, 0][tetv - 1].mean(axis=1)
        slab = np.clip((u * 7).astype(np.int32), 0, 6)
        rng = np.random.default_rng(3)
        isl = slab.copy()
        isl[rng.integers(0, ne, 400)] = rng.integers(0, 7, 400).astype(np.int32)
        head, flag = ctx.empty((ne,), np.int32), ctx.empty((ne,), np.int32)
        for name, part, nc, kw in (("one", None, 1, dict(adja=da)), ("slabs", slab, 7, dict(adja=da)),
                                   ("islands", isl, 7, dict(adja=da)), ("islands packed", isl, 7, dict(tet8=d8)),
                                   ("islands built", isl, 7, dict())):
            dp = None if part is None else ctx.upload(part)
            r = ctx.part_subgroups(None if kw else dt, part=dp, ncolor=nc, head=head, flag=flag, **kw)
            print("part_subgroups", name, r["sub"].shape, sha(r["sub"]), list(r["ncomp"]), r["rounds"],
                  sha(head.download()), sha(flag.download()))
            if part is not None:
                f = ctx.fix_contiguity(None if kw else dt, dp, nc, **kw)
                print("fix_contiguity", name, {k: v for k, v in f.items() if k != "passes"}, sha(dp.download()))
        qual, mn = ctx.tetra_qual(dx, dt)
        print("tetra_qual", mn, sha(qual.download()))
        print("qual_histo", ctx.qual_histo(dt, qual))
        print("mesh_stats_bytes after qual_histo", ctx.mesh_stats_bytes())
        print("edge_lengths", ctx.edge_lengths(dx, dt, dm))
        print("mesh_stats_bytes after edge_lengths without lists", ctx.mesh_stats_bytes())
        r, e, l = ctx.edge_lengths(dx, dt, dm, want_edges=True)
        print("edge_lengths lists", e.shape, sha(e.download()), sha(l.download()))
        print("mesh_stats_bytes after edge_lengths with lists", ctx.mesh_stats_bytes())
        ctx.release_scratch()
        print("mesh_stats_bytes after release_scratch", ctx.mesh_stats_bytes())
        print("edge_lengths again", ctx.edge_lengths(dx, dt, dm) == r)
        x, a, w = ctx.metis_graph(dx, dt, adja=da, met=dm)
        print("metis_graph after release", sha(x.download()), sha(a.download()), sha(w.download()))


if __name__ == "__main__":
    print("build:", os.path.basename(os.environ.get("PMMG_HIP_SO", "tree")))
    refusals()
    results()
