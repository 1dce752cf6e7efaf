"""Outputs and counters of two builds of libpmmg_hip.so on the same seeded
inputs (runs on the MI355X): cfg3 in input order, under a seeded shuffle
(Morton path), with packed records in and out and with a point map (both
orders), the 10-group call at cfg2 size, and two workloads for the exhaustive
searches under PMMG_HIP_MAXSTEP=1 (the inputs of
tests/test_gpu_fallback_scale.py and the largest case of
tests/test_gpu_fallback_edges.py with a tensor field added, each with arrays
and with packed records);
two calls per workload on one context.  Each build runs in a child process of
its own, loaded through PMMG_HIP_SO.

  python tools/identity_ab.py A.so B.so OUT.txt    one child per build, then the comparison (exit 0: identical)
  python tools/identity_ab.py child OUT.json       one build: SHA-256 of every output array, and the counters
"""
import hashlib
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(1, os.path.join(ROOT, "tests"))  # the fallback workloads are the tests' inputs


def sha(a):
    import numpy as np
    return hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()


def child(out_path):
    import numpy as np
    from bench import build_workload
    from parmmg_amd import configs, synth
    from parmmg_amd.transfer import TransferContext, pack_solutions, pack_tet8

    res = {}

    def counters(st):
        return {k: v for k, v in st.as_dict().items() if not k.startswith("ms_")}

    def workload(bg, met, fields, hausd, nq, sort=None):
        """A context with the background and the solutions on the device; returns it and run(name, queries,
        classes, packed, src): two calls, their outputs' checksums and counters into res"""
        ctx = TransferContext(0, sort=sort)
        d = dict(xyz=ctx.upload(bg.xyz), tet8=ctx.upload(pack_tet8(bg.tetv, bg.adja)), triv=ctx.upload(bg.triv),
                 adjt=ctx.upload(bg.adjt), met=ctx.upload(met), f=[ctx.upload(f) for f in fields],
                 rec=ctx.upload(pack_solutions(met, fields)))
        mo = ctx.empty((nq, 6), np.float64)
        fo = [ctx.empty((nq, f.shape[1]), np.float64) for f in fields]
        el, hit = ctx.empty((nq,), np.int32), ctx.empty((nq,), np.int8)
        ro = ctx.empty((nq, d["rec"].shape[1]), np.float64)

        def run(name, q, c, packed=False, src=None):
            dq, dc = ctx.upload(q), ctx.upload(c)
            dsrc = None if src is None else ctx.upload(src)
            for call in range(2):
                for a in [mo, el, hit, ro] + fo:
                    a.zero()
                ctx.set_background_tet8(d["xyz"], d["tet8"], d["triv"], d["adjt"], hausd)
                if packed:
                    ctx.set_solutions_packed(d["rec"], 6, [f.shape[1] for f in fields])
                else:
                    ctx.set_solutions(d["met"], d["f"])
                if dsrc is not None:
                    ctx.set_point_map(dsrc)
                if packed:
                    st = ctx.locate_interp_rec(dq, dc, ro, el, hit)
                    arrays = dict(rec=ro.download())
                else:
                    st = ctx.locate_interp(dq, dc, mo, fo, el, hit)
                    arrays = dict(met=mo.download(), **{f"f{j}": f.download() for j, f in enumerate(fo)})
                arrays.update(elem=el.download(), hit=hit.download())
                res[f"{name}/call{call}"] = dict(arrays={k: sha(v) for k, v in arrays.items()}, stats=counters(st))
            for a in (dq, dc) + (() if dsrc is None else (dsrc,)):
                a.free()
            return arrays

        return ctx, run

    w = configs.CFG3
    bg, new, met, fields, pc = build_workload(w, 0)
    nq = new.np
    ctx, run = workload(bg, met, fields, w.hausd, nq)
    perm = np.random.default_rng(11).permutation(nq)
    src_of = {}
    out = run("cfg3 input order", new.xyz, pc)
    src_of["input"] = synth.point_map(bg, new.xyz, elem=out["elem"], pclass=pc)
    run("cfg3 packed records in and out", new.xyz, pc, packed=True)
    run("cfg3 point map", new.xyz, pc, src=src_of["input"])
    qs, cs = np.ascontiguousarray(new.xyz[perm]), np.ascontiguousarray(pc[perm])
    run("cfg3 shuffled (Morton)", qs, cs)
    run("cfg3 shuffled, packed records in and out", qs, cs, packed=True)
    run("cfg3 shuffled, point map", qs, cs, src=np.ascontiguousarray(src_of["input"][perm]))
    ctx.close()
    del bg, new, met, fields

    # the exhaustive searches: every walk stopped after one step (read when the context is created); the
    # tests' solutions and a tensor field, the layout packed records are compiled for
    import test_gpu_fallback_edges as edges
    import test_gpu_fallback_scale as scale
    os.environ["PMMG_HIP_MAXSTEP"] = "1"
    try:
        bg = synth.lattice(synth.CUBE, scale.N_OLD)
        met = synth.solution(synth.F_ANI, bg.xyz)
        fields = [synth.solution(f, bg.xyz) for f in (synth.F_SCALAR, synth.F_VECTOR, synth.F_TENSOR)]
        xyz, pc = scale._queries(np.random.default_rng(2025), n_in=2000, n_out=400, n_face=2000, n_far=300)
        ctx, run = workload(bg, met, fields, scale.HAUSD, xyz.shape[0], sort=False)
        run("fallbacks at scale (1.05M tetra, 4700 queries)", xyz, pc)
        run("fallbacks at scale, packed records in and out", xyz, pc, packed=True)
        ctx.close()
        case = edges.edge_case(edges.VOL_OUT[-1], edges.BDY_FAR[-1])[0]
        fields = case["fields"] + [synth.solution(synth.F_TENSOR, case["bg"].xyz)]
        ctx, run = workload(case["bg"], case["met"], fields, case["hausd"], case["new"].np, sort=False)
        run("fallback edges (384 tetra, 16385 outside, 8193 far)", case["new"].xyz, case["pclass"])
        run("fallback edges, packed records in and out", case["new"].xyz, case["pclass"], packed=True)
        ctx.close()
    finally:
        del os.environ["PMMG_HIP_MAXSTEP"]
    del bg, met, fields, case

    w = configs.CFG2
    ctx = TransferContext(0)
    gs = []
    for i in range(10):
        bg, new, met, fields, pc = build_workload(w, 100 + i)
        n = new.np
        gs.append(dict(xyz=ctx.upload(bg.xyz), tet8=ctx.upload(pack_tet8(bg.tetv, bg.adja)), triv=ctx.upload(bg.triv),
                       adjt=ctx.upload(bg.adjt), hausd=w.hausd, met=ctx.upload(met),
                       fields=[ctx.upload(f) for f in fields], xyz_new=ctx.upload(new.xyz), pclass=ctx.upload(pc),
                       met_out=ctx.empty((n, w.met_size), np.float64),
                       fields_out=[ctx.empty((n, f.shape[1]), np.float64) for f in fields],
                       elem_out=ctx.empty((n,), np.int32), hit_out=ctx.empty((n,), np.int8)))
    for call in range(2):
        for g in gs:
            for a in [g["met_out"], g["elem_out"], g["hit_out"]] + g["fields_out"]:
                a.zero()
        st = ctx.locate_interp_groups(gs, sync=True)
        arrays = {}
        for i, g in enumerate(gs):
            arrays[f"g{i}.met"] = sha(g["met_out"].download())
            arrays[f"g{i}.f0"] = sha(g["fields_out"][0].download())
            arrays[f"g{i}.elem"] = sha(g["elem_out"].download())
            arrays[f"g{i}.hit"] = sha(g["hit_out"].download())
        res[f"10 groups at cfg2 size/call{call}"] = dict(arrays=arrays, stats=counters(st))
    ctx.close()
    with open(out_path, "w") as f:
        json.dump(res, f, indent=1, sort_keys=True)


def main():
    if sys.argv[1] == "child":
        child(sys.argv[2])
        return 0
    so_a, so_b, out_txt = sys.argv[1:4]
    got = []
    for tag, so in (("A", so_a), ("B", so_b)):
        js = os.path.join(os.path.dirname(out_txt), f"identity_{tag}.json")
        env = dict(os.environ, PMMG_HIP_SO=os.path.abspath(so))
        r = subprocess.run([sys.executable, os.path.abspath(__file__), "child", js], env=env, timeout=420)
        if r.returncode != 0:
            print(f"child {tag} ({so}) ended with status {r.returncode}: stopping")
            return r.returncode or 1
        got.append(json.load(open(js)))
    a, b = got
    lines = [f"A = {so_a}", f"B = {so_b}",
             "every output array (SHA-256 of its bytes), elem, hit and every pmmg_hip_stats counter but ms_*;",
             "two calls per workload on one context (the second on the first's scratch and refilled seed grids)", ""]
    bad = 0
    for key in sorted(a):
        same = a[key] == b.get(key)
        bad += not same
        s = a[key]["stats"]
        lines.append(f"{'IDENTICAL' if same else 'DIFFERENT':12s} {key:56s} {len(a[key]['arrays'])} arrays  "
                     f"sorted={s['sorted']} nvol={s['nvol']} nbdy={s['nbdy']} exact={s['nvol_exact']} "
                     f"vol_exh={s['nvol_exhaust']} vol_closest={s['nvol_closest']} bdy_exh={s['nbdy_exhaust']} "
                     f"bdy_closest+stale={s['nbdy_closest'] + s['nbdy_stale']} src={s['nvol_src']}/{s['nbdy_src']}")
    bad += set(a) != set(b)
    lines += ["", "RESULT: all workloads byte-identical" if not bad else f"RESULT: {bad} workloads DIFFER"]
    open(out_txt, "w").write("\n".join(lines) + "\n")
    print("\n".join(lines))
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
