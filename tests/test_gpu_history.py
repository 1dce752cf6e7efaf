"""A context carries state from call to call — work buffers sized by the
largest call, the fallback lists and their counters, seed grids left "clean"
for the next call, start tables, group lanes, the slot layout of the last
solutions — and none of it may show in a result (runs on the MI355X).

test_call_sequence: nine different calls on one context, each bit-identical
to the same call on a fresh context, in both forced orders.

test_refilled_seed_grids: from 2^20 cells on, a call refills its seed grids
at its end and the next call skips clearing them (ng_clr == 0 / nsg_clr == 0
in run_device).  With PMMG_HIP_TPC=1 and PMMG_HIP_SRFMULT=64 the cube lattice
n_old = 57 (1,111,158 tetra, 38,988 trias) is the smallest to reach that
(g = 103, gs = 107).  The sequence A, B (a smaller grid in the same buffer:
ng_clr == 0 with fewer cells), A, A with a point map that covers every point
(the volume grid is neither filled nor read, and refilled all the same), A
executes every combination of clean / dirty and larger / smaller; each call
is bit-identical to its fresh-context run.

test_every_buffer_family_then_destroy: a context that has used every family
of device buffers it owns (copies of host inputs, a device-built background,
host-mode staging, field vectors that shrink, two kept slots and a consumed
carry-over, packed records, a point map and its start tables, group lanes, the
reports' and the graph's scratch) is destroyed as it stands, and the next
context of the process starts from nothing."""
import numpy as np
import pytest

from parity import (HIT_COUNTERS, assert_skipped_keep, assert_stats_match, check, make_case, make_ctx, outside_case,
                    run_gpu, same_outputs)
from parmmg_amd import synth
from parmmg_amd.transfer import TransferContext
from test_gpu_groups import _device_group, _download
from test_gpu_parity import _packed_variant

C, S = synth.CUBE, synth.SHELL
# the hit kinds, and the walks' lengths: a walk is a function of its query and its seed, so a seed grid that
# kept cells of an earlier call shows in the step counts even where every walk still arrives
COUNTERS = ["nvol", "nbdy", "sorted", "nvol_src", "nbdy_src", "steps_total", "stepmax", "nvol_noseed",
            "nvol_exact"] + list(HIT_COUNTERS.values())


def run_mapped(case, ctx, src=None, tet8=True):
    """run_gpu with an optional armed point map"""
    if src is None:
        return run_gpu(case, ctx=ctx, tet8=tet8)
    bg, new = case["bg"], case["new"]
    from parmmg_amd.transfer import pack_tet8
    ctx.set_background_tet8(bg.xyz, pack_tet8(bg.tetv, bg.adja), bg.triv, bg.adjt, case["hausd"])
    ctx.set_solutions(case["met"], case["fields"])
    ctx.set_point_map(src)
    n = new.np
    met = None if case["met"] is None else np.full((n, case["met"].shape[1]), np.nan)
    fo = [np.full((n, f.shape[1]), np.nan) for f in case["fields"]]
    el, hit = np.zeros(n, np.int32), np.zeros(n, np.int8)
    st = ctx.locate_interp(new.xyz, case["pclass"], met, fo, el, hit)
    return dict(met=met, fields=fo, elem=el, hit=hit, stats=dict(st.as_dict(), reserved=list(st.reserved)))


def run_groups(cases, ctx):
    gs = [_device_group(ctx, c, tet8=(i == 0)) for i, c in enumerate(cases)]
    st = ctx.locate_interp_groups(gs, sync=True)
    outs = [_download(g) for g in gs]
    for g in gs:
        for a in g.values():
            for b in (a if isinstance(a, list) else [a]):
                if hasattr(b, "free"):
                    b.free()
    return outs, dict(st.as_dict(), reserved=list(st.reserved))


def same_call(a, b):
    same_outputs(a, b)
    for key in COUNTERS:
        assert a["stats"][key] == b["stats"][key], (key, a["stats"][key], b["stats"][key])


@pytest.fixture(scope="module")
def seq_cases():
    shell = make_case(kind=S, n_old=8, n_new=12, req_every=5)
    outside = outside_case()
    packed = _packed_variant(make_case(kind=C, n_old=10, n_new=13, jitter_old=0.15, req_every=6, with_ref=False))
    # no boundary trias: nt = 0, the surface points skipped
    import dataclasses
    nob = make_case(kind=C, n_old=6, n_new=7, with_ref=False)
    nob["bg"] = dataclasses.replace(nob["bg"], triv=np.zeros((0, 3), np.int32), adjt=np.zeros((0, 3), np.int32))
    nob["pclass"] = np.where(nob["pclass"] == 2, 0, nob["pclass"]).astype(np.uint8)
    from oracle import oracle as O
    nob["B"] = O.Background(nob["bg"], nob["met"], nob["fields"], nob["hausd"])
    iso = make_case(kind=C, n_old=6, n_new=7, metric=synth.F_ISO, fields=(synth.F_SCALAR,), req_every=4,
                    with_ref=False)
    mapped = make_case(kind=C, n_old=6, n_new=7, req_every=8, with_ref=False)
    mapped["src"] = synth.point_map(mapped["bg"], mapped["new"].xyz)
    groups = [make_case(kind=C, n_old=7, n_new=5, metric=synth.F_ISO, fields=(synth.F_SCALAR,), with_ref=False),
              make_case(kind=S, n_old=8, n_new=8, with_ref=False)]
    return dict(shell=shell, outside=outside, packed=packed, nob=nob, iso=iso, mapped=mapped, groups=groups)


@pytest.mark.gpu
@pytest.mark.parametrize("sort", [False, True], ids=["input", "morton"])
def test_call_sequence(seq_cases, sort):
    """shell with array solutions, the fallback case, packed records, a
    background without trias, an iso metric with one scalar, an armed point
    map, a groups call, release_scratch, the first call again — on one
    context.  Every call's elem, hit, rows and counters equal the fresh
    context's; skipped rows keep their fill.  A stale list count, a work
    buffer sized by an earlier call or a slot layout left behind shows here."""
    K = seq_cases
    calls = [
        ("shell", lambda ctx: run_gpu(K["shell"], ctx=ctx)),
        ("outside", lambda ctx: run_gpu(K["outside"], ctx=ctx)),
        ("packed", lambda ctx: run_gpu(K["packed"], ctx=ctx, tet8=True, packed=True)),
        ("nob", lambda ctx: run_gpu(K["nob"], ctx=ctx)),
        ("iso", lambda ctx: run_gpu(K["iso"], ctx=ctx, tet8=True)),
        ("mapped", lambda ctx: run_mapped(K["mapped"], ctx, K["mapped"]["src"])),
        ("groups", lambda ctx: run_groups(K["groups"], ctx)),
        ("release", lambda ctx: ctx.release_scratch()),
        ("shell", lambda ctx: run_gpu(K["shell"], ctx=ctx)),
    ]
    fresh = {}
    for name, fn in calls:
        if name not in fresh and name != "release":
            with TransferContext(0, sort=sort) as ctx:
                fresh[name] = fn(ctx)
    # the fresh runs meet the contract and their counters their hit arrays
    for name in ("shell", "outside", "packed", "nob", "iso", "mapped"):
        case, out = K[name], fresh[name]
        rep = check(case, out)
        assert rep["n"] == int((case["pclass"] != 0).sum()) and rep["class_i"] == rep["class_i_same"]
        assert_stats_match(out["stats"], case["pclass"], out["hit"], sort=sort)
        assert_skipped_keep(case, out)
    outs, st = fresh["groups"]
    assert_stats_match(st, [c["pclass"] for c in K["groups"]], [o["hit"] for o in outs], sort=sort)
    assert fresh["outside"]["stats"]["nvol_exhaust"] + fresh["outside"]["stats"]["nvol_closest"] > 0
    assert fresh["mapped"]["stats"]["nvol_src"] > 0
    assert fresh["nob"]["stats"]["nbdy"] == 0
    with TransferContext(0, sort=sort) as ctx:
        for i, (name, fn) in enumerate(calls):
            got = fn(ctx)
            if name == "release":
                continue
            if name == "groups":
                for a, b in zip(got[0], fresh[name][0]):
                    same_outputs(a, b)
                for key in COUNTERS:
                    assert got[1][key] == fresh[name][1][key], (i, key)
                continue
            try:
                same_call(got, fresh[name])
            except AssertionError as e:
                raise AssertionError(f"call {i} ({name}) differs from its fresh-context run: {e}") from e
            assert_skipped_keep(K[name], got)


# ---------------------------------------------------------------- every buffer family, then destroy

def host_built(ctx, xyz, tetv, met, fields, new_xyz, pclass, hausd):
    """one host-mode call whose adjacency and boundary trias are built on the
    device (adja absent, nt < 0)"""
    ctx.set_background(xyz, tetv, None, None, None, hausd)
    ctx.set_solutions(met, fields)
    n = new_xyz.shape[0]
    mo = None if met is None else np.full((n, met.shape[1]), np.nan)
    fo = [np.full((n, f.shape[1]), np.nan) for f in fields]
    el, hit = np.zeros(n, np.int32), np.zeros(n, np.int8)
    st = ctx.locate_interp(new_xyz, pclass, mo, fo, el, hit)
    return dict(met=mo, fields=fo, elem=el, hit=hit, stats=dict(st.as_dict(), reserved=list(st.reserved)))


def run_reports(ctx, case):
    """tetra_qual, qual_histo and edge_lengths (with its lists) of a case's background"""
    d = [ctx.upload(case["bg"].xyz), ctx.upload(case["bg"].tetv), ctx.upload(case["met"])]
    qual, mn = ctx.tetra_qual(d[0], d[1], d[2])
    histo = ctx.qual_histo(d[1], qual)
    lens, edges, ll = ctx.edge_lengths(d[0], d[1], d[2], want_edges=True)
    out = dict(qual=qual.download(), minqual=mn, histo=histo, lens=lens, edges=edges.download(), ll=ll.download())
    for a in d + [qual, edges, ll]:
        a.free()
    return out


def run_graph(ctx, case):
    """metis_graph with the adjacency built on the device"""
    d = [ctx.upload(case["bg"].xyz), ctx.upload(case["bg"].tetv), ctx.upload(case["met"])]
    g = ctx.metis_graph(d[0], d[1], met=d[2])
    out = [a.download() for a in g]
    for a in d + list(g):
        a.free()
    return out


def same_report(a, b):
    assert a.keys() == b.keys()
    for key in a:
        if isinstance(a[key], np.ndarray):
            np.testing.assert_array_equal(a[key].view(np.uint8), b[key].view(np.uint8), err_msg=key)
        else:
            assert repr(a[key]) == repr(b[key]), (key, a[key], b[key])  # (repr: NaN equal to itself, -0.0 not to 0.0)


@pytest.mark.gpu
def test_every_buffer_family_then_destroy(seq_cases):
    """On one context: a host-mode call on a device-built background with a
    metric and two fields, kept in slot 0; a host-mode call with one scalar
    field (the field vectors shrink from two to one), kept in slot 1; slot 0
    carried into the next host-mode background and solutions; packed records;
    a point map; two groups; the two reports; the element graph on a
    device-built adjacency.  Every call equals the same call on a fresh
    context.  The context is then destroyed without release_scratch, with
    every buffer family live, and a new context repeats the first call."""
    K = seq_cases
    first = make_case(kind=C, n_old=6, n_new=7, fields=(synth.F_SCALAR, synth.F_VECTOR), req_every=5, with_ref=False)
    iso = K["iso"]
    nxt = make_case(kind=C, n_old=6, n_new=8, req_every=7, with_ref=False)  # (its new points: the carried call's)
    A = first["new"]

    def call_first(ctx):
        return host_built(ctx, first["bg"].xyz, first["bg"].tetv, first["met"], first["fields"], A.xyz,
                          first["pclass"], first["hausd"])

    def call_iso(ctx):
        return host_built(ctx, iso["bg"].xyz, iso["bg"].tetv, iso["met"], iso["fields"], iso["new"].xyz,
                          iso["pclass"], iso["hausd"])

    def call_carried(ctx, rows):
        # the adapted mesh of the first call is the old mesh now; the host holds the rows the step wrote and
        # fills the others (skipped points) itself
        met, fields = rows["met"].copy(), [f.copy() for f in rows["fields"]]
        skip = np.isnan(met[:, 0])
        met[skip] = [1.0, 0.0, 0.0, 1.0, 0.0, 1.0]
        for f in fields:
            f[np.isnan(f[:, 0])] = -2.0
        return host_built(ctx, A.xyz, A.tetv, met, fields, nxt["new"].xyz, nxt["pclass"], first["hausd"])

    with TransferContext(0) as ctx:
        f_first = call_first(ctx)
    assert (first["pclass"] == 0).any() and np.isnan(f_first["met"][first["pclass"] == 0]).all()
    assert f_first["stats"]["nvol"] > 0 and f_first["stats"]["nbdy"] > 0
    fresh = dict(first=f_first)
    for name, fn in (("iso", call_iso), ("carried", lambda c: call_carried(c, f_first)),
                     ("packed", lambda c: run_gpu(K["packed"], ctx=c, tet8=True, packed=True)),
                     ("mapped", lambda c: run_mapped(K["mapped"], c, K["mapped"]["src"])),
                     ("groups", lambda c: run_groups(K["groups"], c)),
                     ("reports", lambda c: run_reports(c, K["shell"])),
                     ("graph", lambda c: run_graph(c, K["shell"]))):
        with TransferContext(0) as ctx:
            fresh[name] = fn(ctx)
    assert fresh["carried"]["stats"]["nvol"] > 0 and fresh["mapped"]["stats"]["nvol_src"] > 0
    assert fresh["reports"]["lens"]["nedge"] > 0 and fresh["graph"][0][-1] > 0

    ctx = TransferContext(0)
    try:
        same_call(call_first(ctx), fresh["first"])
        ctx.keep(0)
        same_call(call_iso(ctx), fresh["iso"])
        ctx.keep(1)
        ctx.carry_over(0, A.np)
        same_call(call_carried(ctx, fresh["first"]), fresh["carried"])
        with pytest.raises(RuntimeError, match="holds nothing"):
            ctx.carry_over(0, A.np)  # consumed by the call above
        same_call(run_gpu(K["packed"], ctx=ctx, tet8=True, packed=True), fresh["packed"])
        same_call(run_mapped(K["mapped"], ctx, K["mapped"]["src"]), fresh["mapped"])
        outs, st = run_groups(K["groups"], ctx)
        for a, b in zip(outs, fresh["groups"][0]):
            same_outputs(a, b)
        for key in COUNTERS:
            assert st[key] == fresh["groups"][1][key], key
        same_report(run_reports(ctx, K["shell"]), fresh["reports"])
        for a, b in zip(run_graph(ctx, K["shell"]), fresh["graph"]):
            np.testing.assert_array_equal(a, b)
        assert ctx.mesh_stats_bytes() > 0
    finally:
        ctx.close()  # pmmg_hip_destroy, no release_scratch before it
    with TransferContext(0) as ctx:
        same_call(call_first(ctx), fresh["first"])


# ---------------------------------------------------------------- refilled seed grids

GRID_ENV = {"PMMG_HIP_TPC": "1", "PMMG_HIP_SRFMULT": "64"}


def random_case(n_old, nq, seed):
    """the cube lattice n_old with nq random queries: four in five inside,
    one in five on a face of the cube (surface points)"""
    from oracle import oracle as O
    bg = synth.lattice(C, n_old)
    rng = np.random.default_rng(seed)
    xyz = rng.random((nq, 3))
    pc = np.ones(nq, np.uint8)
    srf = np.arange(nq) % 5 == 4
    ax, side = rng.integers(0, 3, nq), rng.integers(0, 2, nq).astype(np.float64)
    xyz[srf, ax[srf]] = side[srf]
    pc[srf] = 2
    pc[::13] = 0
    new = synth.Mesh(C, 0, np.ascontiguousarray(xyz), np.zeros((0, 4), np.int32), np.zeros((0, 4), np.int32),
                     np.zeros((0, 3), np.int32), np.zeros((0, 3), np.int32), (pc == 2).astype(np.uint8))
    met = synth.solution(synth.F_ANI, bg.xyz)
    fs = [synth.solution(synth.F_SCALAR, bg.xyz), synth.solution(synth.F_VECTOR, bg.xyz)]
    return dict(bg=bg, new=new, met=met, fields=fs, pclass=pc, hausd=0.01, B=O.Background(bg, met, fs, 0.01))


@pytest.fixture(scope="module")
def grid_cases():
    return dict(A=random_case(57, 20000, 1), B=random_case(40, 5000, 2))


@pytest.mark.gpu
def test_refilled_seed_grids(grid_cases):
    """A, B, A, A + map, A on one context (see the module's text): call 1
    (B) takes ng_clr == 0 and nsg_clr == 0 with smaller grids in A's refilled
    buffers — the branch no other test enters — and leaves them dirty, so
    call 2 clears both again; calls 3 and 4 skip the clearing at the same
    size, call 3 (every volume walk from the map, nvol_src == nvol) without
    filling or reading the volume grid before it is refilled.  Each call equals its
    fresh-context run bit for bit, hit kinds and step counts included; A is
    checked against the oracle on 1500 points."""
    A, B = grid_cases["A"], grid_cases["B"]
    assert A["bg"].ne == 1111158 and A["bg"].nt == 38988  # g = 103, gs = 107: both grids from 2^20 cells on
    assert int(np.cbrt(A["bg"].ne)) ** 3 >= 1 << 20 > int(np.cbrt(B["bg"].ne)) ** 3

    def fresh(case, src=None):
        with make_ctx(env=GRID_ENV) as ctx:
            return run_mapped(case, ctx, src)

    fa, fb = fresh(A), fresh(B)
    rep = check(A, fa, max_points=1500)
    assert rep["n"] == 1500
    for case, out in ((A, fa), (B, fb)):
        assert_stats_match(out["stats"], case["pclass"], out["hit"], sort=False)
        assert_skipped_keep(case, out)
    # a map that covers every point: the nearest vertex of the element found
    src = synth.point_map(A["bg"], A["new"].xyz, elem=fa["elem"], pclass=A["pclass"])
    assert (src[A["pclass"] != 0] > 0).all()
    fm = fresh(A, src)
    st = fm["stats"]
    assert st["nvol_src"] == st["nvol"]  # no volume query needs the seed grid
    assert_stats_match(st, A["pclass"], fm["hit"], sort=False)
    seq = [("A", A, None, fa), ("B", B, None, fb), ("A", A, None, fa), ("A+map", A, src, fm), ("A", A, None, fa)]
    with make_ctx(env=GRID_ENV) as ctx:
        for i, (name, case, m, want) in enumerate(seq):
            got = run_mapped(case, ctx, m)
            try:
                same_call(got, want)
            except AssertionError as e:
                raise AssertionError(f"call {i} ({name}) differs from its fresh-context run: {e}") from e
