"""The device's wedge and cone tests (tri_wedge, tri_cone, cone_tria,
tri_cone_scan of pmmg_device.hpp, the visited-neighbour logic of bdy_query)
against their definition on the surface zoo of tests/surface_ref.py: ridges
of five dihedral angles, closed fans across kFanMax with no environment
setting, one rejecting edge at every rotation position, open and non-manifold
fans, pinched vertices, fans with trias stored in either orientation.  The
CPU oracle meets the same definition from three starts per query in
test_surface_ref_host.py.

With a point map every walk starts in a chosen tria of the query's home
(k_bdy<1>); without one the seed grid chooses (k_bdy<0>): the nearest recorded
centroid among the cells around the query.  The patches lie 4.0 apart and a
query within 1.3 of every centroid of its own patch; with the grid sized as it
is for 765 trias the seed is a tria of the query's patch for every one of the
121 queries (MI355X), though at a pinched vertex or a non-manifold edge it may
belong to another fan or sheet than the one the query was made for.  The
second run therefore accepts the definition from any home of the query's
patch, and nothing else: the oracle's answers do not depend on the start
within a home.  (A seed grid that left a zoo query without a seed, or with one
from another patch, would send it to the exhaustive search and fail here.)

One deviation is pinned: at a pinched vertex the device
tests the fan the walk stands in, the reference every tria of the vertex."""
import dataclasses

import numpy as np
import pytest

import highprec_interp as HI
import surface_ref as SR
from oracle import oracle as O
from parity import VIEW_OFFSETS, assert_stats_match, check, device_view, make_ctx
from parmmg_amd import synth
from parmmg_amd.transfer import pack_tet8

NAMES = (SR.METRIC,) + SR.FIELDS


@pytest.fixture(scope="module")
def case():
    Z = SR.zoo()
    bg, B = SR.background(Z)
    e4, e3 = np.zeros((0, 4), np.int32), np.zeros((0, 3), np.int32)
    new = synth.Mesh(synth.CUBE, 0, Z["q"], e4, e4, e3, e3, None)
    return dict(Z=Z, bg=bg, new=new, met=Z["sol"][SR.METRIC], fields=[Z["sol"][f] for f in SR.FIELDS],
                pclass=Z["pclass"], B=B, hausd=SR.HAUSD)


def subset(case, idx):
    """the case with the queries idx only"""
    idx = np.asarray(idx, np.int64)
    new = dataclasses.replace(case["new"], xyz=np.ascontiguousarray(case["new"].xyz[idx]))
    return dict(case, new=new, pclass=np.ascontiguousarray(case["pclass"][idx]))


def run(case, src=None, sort=False, device=False):
    """one transfer of the case's queries; device: every array in device memory, triv and adjt between guard
    zones, 4 bytes past a 256-byte boundary"""
    bg, q, pc, met, fields = case["bg"], case["new"].xyz, case["pclass"], case["met"], case["fields"]
    n = q.shape[0]
    ctx = make_ctx(sort)
    allocs = []
    try:
        tet8 = pack_tet8(bg.tetv, bg.adja)
        if device:
            triv, a = device_view(ctx, bg.triv, VIEW_OFFSETS["triv"])
            allocs.append(("triv", a))
            adjt, a = device_view(ctx, bg.adjt, VIEW_OFFSETS["adjt"])
            allocs.append(("adjt", a))
            ctx.set_background_tet8(ctx.upload(bg.xyz), ctx.upload(tet8), triv, adjt, case["hausd"])
            ctx.set_solutions(ctx.upload(met), [ctx.upload(f) for f in fields])
            if src is not None:
                ctx.set_point_map(ctx.upload(np.ascontiguousarray(src, np.int32)))
            outs = [ctx.upload(np.full((n, SR.SIZE[name]), np.nan)) for name in NAMES]
            el, hit = ctx.upload(np.zeros(n, np.int32)), ctx.upload(np.zeros(n, np.int8))
            st = ctx.locate_interp(ctx.upload(q), ctx.upload(pc), outs[0], outs[1:], el, hit)
            rows, el, hit = [o.download() for o in outs], el.download(), hit.download()
            for name, a in allocs:
                a.check(name)
        else:
            ctx.set_background_tet8(bg.xyz, tet8, bg.triv, bg.adjt, case["hausd"])
            ctx.set_solutions(met, fields)
            if src is not None:
                ctx.set_point_map(np.ascontiguousarray(src, np.int32))
            rows = [np.full((n, SR.SIZE[name]), np.nan) for name in NAMES]
            el, hit = np.zeros(n, np.int32), np.zeros(n, np.int8)
            st = ctx.locate_interp(q, pc, rows[0], rows[1:], el, hit)
        return dict(met=rows[0], fields=rows[1:], elem=el, hit=hit, stats=dict(st.as_dict(), reserved=list(st.reserved)))
    finally:
        for _, a in allocs:
            a.free()
        ctx.close()


def matches(exp, h, k, loc):
    kind, elems = exp
    return h == kind and k in elems and (kind not in (SR.BDY_WEDGE, SR.BDY_CONE) or loc == elems[k])


def check_zoo(case, out, mapped, what):
    """every query's kind, loc, element and rows against the definition; the rows bit-equal to the oracle's in the
    reported element; the contract of parity.check; the counters.  Returns the queries that took the deviation."""
    Z, B = case["Z"], case["B"]
    code, locs = out["hit"].astype(np.int32) & 15, (out["hit"].astype(np.int32) >> 4) & 3
    worst, deviating, scans_needed, own = {}, [], 0, {SR.BDY_WEDGE: 0, SR.BDY_CONE: 0}
    for qi in range(Z["q"].shape[0]):
        h, k, loc = int(code[qi]), int(out["elem"][qi]), int(locs[qi])
        label = (what, qi, Z["patch"][Z["qpatch"][qi]]["name"], Z["label"][qi], h, k, loc)
        homes = [Z["home"][qi]] if mapped else list(Z["patch"][Z["qpatch"][qi]]["comps"])
        cands = [(SR.define(Z, qi, c), SR.device_define(Z, qi, c)) for c in homes]
        true = next((t for t, d in cands if matches(d, h, k, loc)), None)
        assert true is not None, (label, cands, "no start in the query's patch gives this answer" if not mapped else "")
        if h in own:
            own[h] += 1
        if not matches(true, h, k, loc):
            # the pinned deviation: a cone of the walk's own fan where the vertex's other fan rejects
            assert Z["label"][qi] == "pinched-one-fan" and h == SR.BDY_CONE and true[0] == SR.BDY_CLOSEST, (label, true)
            deviating.append(qi)
        if h == SR.BDY_CONE:
            v = int(Z["triv"][k - 1][loc])
            scans_needed += int(SR.scan_vertex(Z, v))
            assert np.array_equal(out["met"][qi].view(np.uint64), Z["sol"][SR.METRIC][v - 1].view(np.uint64)), label
        got = [out["met"][qi]] + [f[qi] for f in out["fields"]]
        met, fr = O.eval_in_element(B, Z["q"][qi], True, k, h, loc)
        for name, g, w in zip(NAMES, got, [met] + fr):
            assert np.array_equal(g.view(np.uint64), w.view(np.uint64)), (label, name, g, w)
        want = SR.rows(qi, h, k, loc)
        for name, g in zip(NAMES, got):
            ratio, _ = HI.row_ratio(g, *want[name])
            key = (h, "p1" if SR.SIZE[name] < 6 else "tensor")
            worst[key] = max(worst.get(key, 0.0), ratio)
            assert ratio <= 1.0, (label, name, ratio)
    keep = np.setdiff1d(np.arange(Z["q"].shape[0]), deviating)
    sub = dict(met=out["met"][keep], fields=[f[keep] for f in out["fields"]], elem=out["elem"][keep], hit=out["hit"][keep])
    rep = check(subset(case, keep), sub)
    assert rep["n"] == keep.size
    st = out["stats"]
    assert_stats_match(st, case["pclass"], out["hit"])
    assert st["nbdy_src"] == (Z["q"].shape[0] if mapped else 0)
    assert scans_needed <= st["nbdy_fanscan"], (st["nbdy_fanscan"], scans_needed)
    print(what, "hits", np.bincount(code, minlength=12)[4:].tolist(), "fanscan", st["nbdy_fanscan"], ">=", scans_needed,
          "deviating", deviating, "worst error/bound", {f"{a}-{b}": round(v, 3) for (a, b), v in sorted(worst.items())})
    return deviating, own


@pytest.mark.gpu
@pytest.mark.parametrize("device", [False, True], ids=["host", "device"])
@pytest.mark.parametrize("sort", [False, True], ids=["input", "morton"])
def test_zoo_with_a_point_map(case, sort, device):
    """k_bdy<1>: each walk starts in the tria its source vertex names.  Every answer is the definition's; the six
    queries at the pinched vertices that one fan alone admits are cones on the device (the reference: closest)."""
    Z = case["Z"]
    out = run(case, Z["src"], sort, device)
    deviating, _ = check_zoo(case, out, True, f"map {'morton' if sort else 'input'} {'device' if device else 'host'}")
    assert deviating == [qi for qi in range(Z["q"].shape[0]) if Z["label"][qi] == "pinched-one-fan"]
    code = out["hit"].astype(np.int32) & 15
    kinds = np.array([SR.device_define(Z, qi)[0] for qi in range(Z["q"].shape[0])])
    np.testing.assert_array_equal(code, kinds)


@pytest.mark.gpu
@pytest.mark.parametrize("device", [False, True], ids=["host", "device"])
@pytest.mark.parametrize("sort", [False, True], ids=["input", "morton"])
def test_zoo_from_the_seed_grid(case, sort, device):
    """k_bdy<0>: the seed grid chooses the start; wedges and cones are reached by the plain kernel too"""
    out = run(case, None, sort, device)
    _, own = check_zoo(case, out, False, f"nomap {'morton' if sort else 'input'} {'device' if device else 'host'}")
    assert own[SR.BDY_WEDGE] > 0 and own[SR.BDY_CONE] > 0, own


@pytest.mark.gpu
def test_no_scan_at_closed_manifold_fans_up_to_kfanmax(case):
    """a call whose queries all sit at closed manifold fans of at most 64 trias (the rejecting copies and the
    pinched vertices among them) never scans; the whole zoo's scans are counted in check_zoo"""
    Z = case["Z"]
    idx = [qi for qi in range(Z["q"].shape[0])
           if Z["patch"][Z["qpatch"][qi]]["kind"] in ("fan", "reject", "flipped", "pinched")
           and Z["patch"][Z["qpatch"][qi]]["n"] <= SR.FAN_MAX]
    sizes = {Z["patch"][Z["qpatch"][qi]]["n"] for qi in idx}
    assert {3, 12, 63, 64} <= sizes and len(idx) > 60
    sub = subset(case, idx)
    for src in (Z["src"][idx], None):
        out = run(sub, src)
        code = out["hit"].astype(np.int32) & 15
        assert out["stats"]["nbdy_fanscan"] == 0, out["stats"]
        assert (code == SR.BDY_CONE).sum() > 0 and (code == SR.BDY_WEDGE).sum() > 0
        if src is not None:
            np.testing.assert_array_equal(code, [SR.device_define(Z, qi)[0] for qi in idx])
