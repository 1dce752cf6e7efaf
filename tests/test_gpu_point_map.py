"""Point map (Mmg's USE_POINTMAP): pmmg_hip_set_point_map hands the module the
old-mesh vertex each new point descends from (MMG5_Point.src), and the walks
of the armed call start at the element PMMG_locate_setStart
(src/locate_pmmg.c:931-986) derives from it — the first tria holding the
source vertex for a boundary point, the first tetra for a volume point —
instead of at the module's seed grids.

The start tables are checked against a numpy restatement of that function;
mapped calls fall under the parity contract of tests/parity.py (the element
of a class (i) point does not depend on where its walk started), in both
query orders and both output forms, with good, useless and hostile maps."""
import os

import numpy as np
import pytest

from parity import EPS, check, make_case
from parmmg_amd import synth
from parmmg_amd.transfer import TransferContext, pack_solutions, pack_tet8

C, S = synth.CUBE, synth.SHELL
PACKABLE = (synth.F_SCALAR, synth.F_VECTOR, synth.F_TENSOR)  # with the aniso metric: 16 doubles per record
# the cube at n_old = 6 (1296 tetra), n_new = 7; the curved kind at its smallest lattices (the shell needs a
# multiple of 4, at least 8: 2688 tetra)
SPECS = {"cube": dict(kind=C, n_old=6, n_new=7), "shell": dict(kind=S, n_old=8, n_new=12)}


def set_start(npt, tetv, triv):
    """PMMG_locate_setStart restated: per vertex the first tetra / tria that
    holds it in ascending element order (its `if (s) continue` guards), 0 when
    none; tetra not in use (v[0] <= 0) are passed over."""
    st, sr = np.zeros(npt, np.int32), np.zeros(npt, np.int32)
    for k, v in enumerate(tetv, 1):
        if v[0] <= 0:
            continue
        for ip in v:
            if st[ip - 1] == 0:
                st[ip - 1] = k
    for k, v in enumerate(triv, 1):
        for ip in v:
            if sr[ip - 1] == 0:
                sr[ip - 1] = k
    return st, sr


def expected_counts(case, src, tables):
    """(nvol_src, nbdy_src): the points whose source is a vertex of the
    background with a start element of their class"""
    st, sr = tables
    pc = case["pclass"]
    src = np.asarray(src, np.int64)
    ok = (src >= 1) & (src <= st.shape[0])
    s0 = np.where(ok, src, 1) - 1
    return int((ok & (pc == 1) & (st[s0] != 0)).sum()), int((ok & (pc == 2) & (sr[s0] != 0)).sum())


@pytest.fixture(scope="module")
def cases():
    """the shared cases with their oracle runs and start tables (never modified)"""
    out = {}
    for name, spec in SPECS.items():
        case = make_case(**spec, metric=synth.F_ANI, fields=PACKABLE)
        bg = case["bg"]
        case["tables"] = set_start(bg.np, bg.tetv, bg.triv)
        case["src"] = synth.point_map(bg, case["new"].xyz)
        # the identical-element assertion must bite: at least half of the volume points in class (i)
        ref, pc = case["ref"], case["pclass"]
        n_i = int(((pc == 1) & np.isin(ref["hit"], (1, 2)) & (ref["minbary"] > EPS)).sum())
        assert 2 * n_i >= int((pc == 1).sum()), (name, n_i)
        out[name] = case
    return out


class Runner:
    """One context with a case resident on the device; run() makes one call."""

    def __init__(self, case, sort=None, layout="tet8", rec=False, env=None):
        saved = {k: os.environ.get(k) for k in (env or {})}
        os.environ.update(env or {})
        try:
            self.ctx = TransferContext(0, sort=sort)
        finally:
            for k, v in saved.items():
                if v is None:
                    os.environ.pop(k, None)
                else:
                    os.environ[k] = v
        ctx, bg = self.ctx, case["bg"]
        self.case, self.rec = case, rec
        met, fields = case["met"], case["fields"]
        self.sizes = [met.shape[1]] + [f.shape[1] for f in fields]
        xyz = ctx.upload(bg.xyz)
        if layout == "tet8":
            ctx.set_background_tet8(xyz, ctx.upload(pack_tet8(bg.tetv, bg.adja)), ctx.upload(bg.triv),
                                    ctx.upload(bg.adjt), case["hausd"])
        elif layout == "tetv":
            ctx.set_background(xyz, ctx.upload(bg.tetv), ctx.upload(bg.adja), ctx.upload(bg.triv),
                               ctx.upload(bg.adjt), case["hausd"])
        else:  # "devtria": boundary trias and their adjacency built on the device
            ctx.set_background(xyz, ctx.upload(bg.tetv), ctx.upload(bg.adja), None, None, case["hausd"])
        if rec:
            ctx.set_solutions_packed(ctx.upload(pack_solutions(met, fields)), met.shape[1],
                                     [f.shape[1] for f in fields])
        else:
            ctx.set_solutions(ctx.upload(met), [ctx.upload(f) for f in fields])
        self.q, self.pc = ctx.upload(case["new"].xyz), ctx.upload(case["pclass"])

    def run(self, src=None, device_map=False):
        ctx, n = self.ctx, self.case["new"].np
        if src is not None:
            ctx.set_point_map(ctx.upload(np.ascontiguousarray(src, np.int32)) if device_map else src)
        el, hit = ctx.upload(np.zeros(n, np.int32)), ctx.upload(np.zeros(n, np.int8))
        if self.rec:
            rs = (sum(self.sizes) + 1) & ~1
            ro = ctx.upload(np.full((n, rs), np.nan))
            st = ctx.locate_interp_rec(self.q, self.pc, ro, el, hit)
            r, rows, o = ro.download(), [], 0
            for s in self.sizes:
                rows.append(np.ascontiguousarray(r[:, o:o + s]))
                o += s
        else:
            outs = [ctx.upload(np.full((n, s), np.nan)) for s in self.sizes]
            st = ctx.locate_interp(self.q, self.pc, outs[0], outs[1:], el, hit)
            rows = [o.download() for o in outs]
        return dict(met=rows[0], fields=rows[1:], elem=el.download(), hit=hit.download(), stats=st.as_dict())

    def close(self):
        self.ctx.close()


def same_outputs(a, b):
    np.testing.assert_array_equal(a["elem"], b["elem"])
    np.testing.assert_array_equal(a["hit"], b["hit"])
    for x, y in zip([a["met"]] + a["fields"], [b["met"]] + b["fields"]):
        assert np.array_equal(x.view(np.uint64), y.view(np.uint64))


# ---------------------------------------------------------------- 1. start tables

@pytest.mark.gpu
@pytest.mark.parametrize("layout", ["tetv", "tet8", "devtria"])
@pytest.mark.parametrize("kind", ["cube", "shell"])
def test_start_tables_equal_set_start(cases, kind, layout):
    case = cases[kind]
    bg = case["bg"]
    r = Runner(case, layout=layout)
    try:
        st, sr = r.ctx.start_elements()
        triv = bg.triv
        if layout == "devtria":  # the trias the device built, in its (tetra, face) order
            t, _ = r.ctx.build_boundary(bg.np, tetv=r.ctx.upload(bg.tetv), adja=r.ctx.upload(bg.adja))
            triv = t.download()
            assert triv.shape[0] == bg.nt
        want_t, want_r = set_start(bg.np, bg.tetv, triv)
        np.testing.assert_array_equal(st, want_t)
        np.testing.assert_array_equal(sr, want_r)
        assert (st != 0).all() and (sr != 0).any() and (sr == 0).any()  # interior vertices have no tria
    finally:
        r.close()


@pytest.mark.gpu
@pytest.mark.parametrize("tet8", [False, True])
def test_start_tables_pass_over_unused_tetra(tet8):
    """rows with v[0] = 0 are never chosen, and a vertex only they use gets 0"""
    xyz = np.array([[0, 0, 0], [1, 0, 0], [0, 1, 0], [0, 0, 1], [1, 1, 1], [2, 2, 2], [3, 3, 3]], np.float64)
    tetv = np.array([[0, 2, 3, 4],    # unused: would be the first tetra of vertices 2, 3, 4
                     [1, 2, 3, 4],
                     [0, 6, 7, 5],    # unused, the only row with vertices 6 and 7
                     [2, 3, 4, 5],
                     [0, 1, 2, 3]], np.int32)
    adja = np.zeros((5, 4), np.int32)
    triv = np.array([[2, 3, 4], [1, 3, 2]], np.int32)
    adjt = np.zeros((2, 3), np.int32)
    with TransferContext(0) as ctx:
        if tet8:
            ctx.set_background_tet8(xyz, pack_tet8(tetv, adja), triv, adjt, 0.01)
        else:
            ctx.set_background(xyz, tetv, adja, triv, adjt, 0.01)
        st, sr = ctx.start_elements()
    np.testing.assert_array_equal(st, [2, 2, 2, 2, 4, 0, 0])
    np.testing.assert_array_equal(sr, [2, 1, 1, 1, 0, 0, 0])
    want = set_start(7, tetv, triv)
    np.testing.assert_array_equal(st, want[0])
    np.testing.assert_array_equal(sr, want[1])


# ---------------------------------------------------------------- 2. parity with a nearest-vertex map

@pytest.mark.gpu
@pytest.mark.parametrize("rec", [False, True], ids=["arrays", "records"])
@pytest.mark.parametrize("sort", [False, True], ids=["input", "morton"])
@pytest.mark.parametrize("kind", ["cube", "shell"])
def test_nearest_vertex_map_parity(cases, kind, sort, rec):
    case = cases[kind]
    r = Runner(case, sort=sort, rec=rec)
    try:
        out = r.run(case["src"], device_map=rec)
    finally:
        r.close()
    rep = check(case, out)
    assert rep["class_i"] == rep["class_i_same"] and 2 * rep["class_i"] >= int((case["pclass"] == 1).sum())
    nv, nb = expected_counts(case, case["src"], case["tables"])
    assert nv == int((case["pclass"] == 1).sum()) and nb > 0  # every vertex has a tetra; the test must bite
    assert out["stats"]["nvol_src"] == nv
    assert out["stats"]["nbdy_src"] == nb
    assert out["stats"]["sorted"] == int(sort)


# ---------------------------------------------------------------- 3. no map in disguise

@pytest.mark.gpu
@pytest.mark.parametrize("sort", [False, True], ids=["input", "morton"])
def test_zero_map_is_no_map_and_the_map_is_consumed(cases, sort):
    case = cases["shell"]
    r = Runner(case, sort=sort)
    try:
        plain = r.run()
        zero = r.run(np.zeros(case["new"].np, np.int32))
        mapped = r.run(case["src"])
        after = r.run()  # not re-armed: the map was consumed
    finally:
        r.close()
    same_outputs(plain, zero)
    same_outputs(plain, after)
    for out in (plain, zero, after):
        assert out["stats"]["nvol_src"] == 0 and out["stats"]["nbdy_src"] == 0
    assert mapped["stats"]["nvol_src"] > 0
    for key in ("nvol", "nbdy", "nvol_walk", "nbdy_face", "steps_total", "stepmax", "nvol_noseed"):
        assert plain["stats"][key] == zero["stats"][key] == after["stats"][key], key


# ---------------------------------------------------------------- 4. bad and adversarial maps

@pytest.fixture(scope="module")
def case8():
    """the largest background of this file: 3072 tetra, so a straight walk
    from any start stays far below the 1024-step cap"""
    case = make_case(kind=C, n_old=8, n_new=7, metric=synth.F_ANI, fields=PACKABLE)
    case["tables"] = set_start(case["bg"].np, case["bg"].tetv, case["bg"].triv)
    return case


@pytest.mark.gpu
@pytest.mark.parametrize("sort", [False, True], ids=["input", "morton"])
@pytest.mark.parametrize("which", ["permutation", "out-of-range"])
def test_far_and_invalid_sources(case8, which, sort):
    case = case8
    npb, n = case["bg"].np, case["new"].np
    rng = np.random.default_rng(7)
    if which == "permutation":  # valid ids, sources far from their points
        src = (rng.permutation(max(npb, n))[:n] % npb + 1).astype(np.int32)
    else:  # unknown, negative and too large ids among a few valid ones
        src = np.array([0, -1, -(2 ** 31), npb + 1, 2 ** 31 - 1, npb, 1, -npb], np.int64)[np.arange(n) % 8].astype(np.int32)
    r = Runner(case, sort=sort)
    try:
        a = r.run(src)
        b = r.run(src)
    finally:
        r.close()
    same_outputs(a, b)
    rep = check(case, a)
    assert rep["class_i"] == rep["class_i_same"]
    nv, nb = expected_counts(case, src, case["tables"])
    assert a["stats"]["nvol_src"] == nv and a["stats"]["nbdy_src"] == nb
    if which == "out-of-range":
        valid = (src >= 1) & (src <= npb)
        assert nv == int((valid & (case["pclass"] == 1)).sum()) and nv < int((case["pclass"] == 1).sum())


# ---------------------------------------------------------------- 5. map plus fallbacks

@pytest.mark.gpu
@pytest.mark.parametrize("kind", ["cube", "shell"])
def test_map_with_one_step_walks(cases, kind):
    """PMMG_HIP_MAXSTEP=1: the start element is tried, then the exhaustive search"""
    case = cases[kind]
    r = Runner(case, env={"PMMG_HIP_MAXSTEP": "1"})
    try:
        out = r.run(case["src"])
    finally:
        r.close()
    rep = check(case, out)
    assert rep["class_i"] == rep["class_i_same"]
    assert rep["hits"].get(2, 0) > 0 and rep["hits"].get(9, 0) > 0  # VOL_EXHAUST and BDY_EXHAUST
    assert out["stats"]["nvol_src"] == int((case["pclass"] == 1).sum())


# ---------------------------------------------------------------- 6. surface rule

@pytest.mark.gpu
def test_surface_point_with_an_interior_source(cases):
    """A boundary point whose source is an interior vertex has no start tria
    (the reference would start at tria 0): it takes the seed grid and is not
    counted in nbdy_src"""
    case = cases["cube"]
    st, sr = case["tables"]
    interior = np.nonzero(sr == 0)[0] + 1
    assert interior.size > 0
    src = case["src"].copy()
    bdy = case["pclass"] == 2
    src[bdy] = interior[np.arange(int(bdy.sum())) % interior.size]
    r = Runner(case)
    try:
        out = r.run(src)
    finally:
        r.close()
    assert out["stats"]["nbdy_src"] == 0
    assert out["stats"]["nvol_src"] == int((case["pclass"] == 1).sum())
    assert out["stats"]["nbdy"] == int(bdy.sum())
    rep = check(case, out)
    assert rep["class_i"] == rep["class_i_same"]


# ---------------------------------------------------------------- 7. arming rules

@pytest.mark.gpu
def test_np_new_mismatch_disarms(cases):
    case = cases["cube"]
    r = Runner(case)
    try:
        plain = r.run()
        with pytest.raises(RuntimeError, match="point map was armed for"):
            r.run(case["src"][:-1])
        again = r.run()  # the failed call disarmed the map
    finally:
        r.close()
    same_outputs(plain, again)
    assert again["stats"]["nvol_src"] == 0 and again["stats"]["nbdy_src"] == 0


@pytest.mark.gpu
def test_groups_call_ignores_an_armed_map(cases):
    case = cases["cube"]
    r = Runner(case)
    try:
        ctx, bg, n = r.ctx, case["bg"], case["new"].np
        g = dict(xyz=ctx.upload(bg.xyz), tet8=ctx.upload(pack_tet8(bg.tetv, bg.adja)), triv=ctx.upload(bg.triv),
                 adjt=ctx.upload(bg.adjt), hausd=case["hausd"], met=ctx.upload(case["met"]),
                 fields=[ctx.upload(f) for f in case["fields"]], xyz_new=r.q, pclass=r.pc,
                 met_out=ctx.upload(np.full((n, 6), np.nan)),
                 fields_out=[ctx.upload(np.full((n, f.shape[1]), np.nan)) for f in case["fields"]],
                 elem_out=ctx.upload(np.zeros(n, np.int32)), hit_out=ctx.upload(np.zeros(n, np.int8)))

        def _download(g):
            return dict(met=g["met_out"].download(), fields=[f.download() for f in g["fields_out"]],
                        elem=g["elem_out"].download(), hit=g["hit_out"].download())

        r.ctx.locate_interp_groups([g])
        without = _download(g)
        for a in [g["met_out"], g["elem_out"], g["hit_out"]] + g["fields_out"]:
            a.zero()
        r.ctx.set_point_map(case["src"])
        st = r.ctx.locate_interp_groups([g])
        with_map = _download(g)
        assert st.nvol_src == 0 and st.nbdy_src == 0
        same_outputs(without, with_map)
        out = r.run()  # the map is still armed for the context's own next call
        assert out["stats"]["nvol_src"] == int((case["pclass"] == 1).sum())
    finally:
        r.close()


@pytest.mark.gpu
def test_release_scratch_rebuilds_the_tables(cases):
    case = cases["shell"]
    r = Runner(case)
    try:
        a = r.run(case["src"])
        r.ctx.release_scratch()
        b = r.run(case["src"])
        st, sr = r.ctx.start_elements()
    finally:
        r.close()
    same_outputs(a, b)
    assert a["stats"]["nvol_src"] == b["stats"]["nvol_src"] and a["stats"]["nbdy_src"] == b["stats"]["nbdy_src"]
    np.testing.assert_array_equal(st, case["tables"][0])
    np.testing.assert_array_equal(sr, case["tables"][1])


# ---------------------------------------------------------------- 8. host layer

@pytest.mark.gpu
def test_host_layer_with_one_mapped_group(cases):
    from parmmg_amd.transfer import TAG_BDY, interp_metrics_and_fields

    def groups():
        olds, news = [], []
        for case in (cases["cube"], cases["shell"]):
            new = case["new"]
            tag = np.where(new.isbdy == 1, TAG_BDY, 0).astype(np.uint16)
            olds.append(dict(mesh=case["bg"], met=case["met"], fields=case["fields"], hausd=case["hausd"]))
            news.append(dict(xyz=new.xyz, tag=tag, tetv=new.tetv, met=np.full((new.np, 6), np.nan),
                             fields=[np.full((new.np, f.shape[1]), np.nan) for f in case["fields"]], ani=1,
                             elem=np.zeros(new.np, np.int32), hit=np.zeros(new.np, np.int8)))
        return olds, news

    with TransferContext(0) as ctx:
        olds, plain = groups()
        ier, st0 = interp_metrics_and_fields(ctx, olds, plain, input_met=1)
        assert ier == 1 and st0.nvol_src == 0 and st0.nbdy_src == 0
        olds, mapped = groups()
        ier, st1 = interp_metrics_and_fields(ctx, olds, mapped, input_met=1, src=[cases["cube"]["src"], None])
        assert ier == 1
    nv, nb = expected_counts(cases["cube"], cases["cube"]["src"], cases["cube"]["tables"])
    assert st1.nvol_src == nv and st1.nbdy_src == nb  # the second group ran without a map
    for case, g, p in zip((cases["cube"], cases["shell"]), mapped, plain):
        out = dict(met=g["met"], fields=g["fields"], elem=g["elem"], hit=g["hit"])
        rep = check(case, out)
        assert rep["class_i"] == rep["class_i_same"]
        ref = case["ref"]
        ci = np.isin(ref["hit"], (1, 2)) & (ref["minbary"] > EPS) & (case["pclass"] == 1)
        np.testing.assert_array_equal(g["elem"][ci], p["elem"][ci])
        for x, y in zip([g["met"]] + g["fields"], [p["met"]] + p["fields"]):
            assert np.array_equal(x[ci].view(np.uint64), y[ci].view(np.uint64))
    same_outputs(dict(met=mapped[1]["met"], fields=mapped[1]["fields"], elem=mapped[1]["elem"], hit=mapped[1]["hit"]),
                 dict(met=plain[1]["met"], fields=plain[1]["fields"], elem=plain[1]["elem"], hit=plain[1]["hit"]))
