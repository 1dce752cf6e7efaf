"""The device's interpolated rows against their definition in 50-digit
arithmetic (tests/highprec_interp.py), held to the bounds the CPU oracle meets
in test_highprec_interp_host.py.

The soup of disjoint elements forces the element: with a point map naming a
vertex of the query's own element the walk starts and ends there (k_vol<...,
MAP> and k_bdy<1> with their own interpolation code), with a map naming a
vertex of another element, or without one, the exhaustive searches of
pmmg_fallback.hpp find it.  Every row the device writes is compared, none
excluded; rows the definition leaves untouched keep the sentinel."""
import re
from pathlib import Path

import numpy as np
import pytest

import highprec_interp as HI
from parity import make_ctx
from parmmg_amd.transfer import pack_solutions, pack_tet8

SENT = np.frombuffer(np.uint64(0x7FF4A5A5A5A5A5A5).tobytes(), np.float64)[0]
SENT_BITS = np.uint64(0x7FF4A5A5A5A5A5A5)

# kLayouts of pmmg_call.hpp, assembled from the pool: (metric, fields)
POOL = {1: ("s0", "s1", "s2", "s3", "s4"), 3: ("vec",), 6: ("ten6",)}
LAYOUTS = ((6, 1, 3, 6), (6, 1, 3, 6, 1), (1, 1), (1, 1, 1, 1, 1, 1), (1, 1, 1), (6,), (1,), (6, 1), (1, 1, 3, 6), ())
RUNTIME = (3, 1, 6, 3)  # no compiled layout: the runtime variant, without a metric


def names_of(layout, metric=True):
    """(metric solution or None, field solutions) of a layout"""
    used = {1: 0, 3: 0, 6: 0}
    out = []
    for j, c in enumerate(layout):
        if j == 0 and metric:
            out.append("met%d" % c)
        else:
            out.append(POOL[c][used[c] % len(POOL[c])])
            used[c] += 1
    return (out[0], tuple(out[1:])) if (metric and out) else (None, tuple(out))


def packed_forms(layout):
    """PackedLayout::valid() and passes_ok() restated: the gather passes a layout's packed form exists with"""
    k = sum(layout)
    rs = (k + 1) & ~1
    if not (k > 0 and rs <= 16):
        return ()
    ok = []
    for npass in (1, 2):
        if (rs // 2) % npass:
            continue
        pw, off, fits = rs // npass, 0, True
        for c in layout:
            if c == 6 and off // pw != (off + 5) // pw:
                fits = False
            off += c
        if fits:
            ok.append(npass)
    return tuple(ok)


def test_layout_list_is_the_kernels():
    """A layout added to kLayouts cannot go untested (CPU: no kernel runs).  packed_forms restates
    PackedLayout::valid() and passes_ok() and is held here to hand-worked cases only; a later change to either
    shows only through the GPU runs below: a layout that leaves the packed set is refused by set_solutions_packed."""
    src = (Path(__file__).resolve().parents[1] / "parmmg_amd" / "csrc" / "pmmg_call.hpp").read_text()
    table = src[src.index("const LayoutEntry kLayouts[]"):]
    table = table[:table.index("};")]
    got = [tuple(int(x) for x in m.groups() if int(x) > 0)
           for m in re.finditer(r"PMMG_LAYOUT\((\d+), (\d+), (\d+), (\d+), (\d+), (\d+)\)", table)]
    assert got == list(LAYOUTS)
    assert packed_forms((6, 1, 3, 6)) == (1, 2) and packed_forms((6,)) == (1,) and packed_forms(()) == ()
    assert packed_forms((1, 1, 3, 6)) == (1,) and packed_forms((1, 1, 1, 1, 1, 1)) == (1,)
    assert packed_forms((6, 1, 3, 6, 1)) == () and packed_forms((1, 1)) == (1,) and packed_forms((6, 1)) == (1,)


def run_soup(fi, metric, fields, form="arrays", route="map", sort=False):
    """one transfer of the soup in FRAMES[fi]: rows per solution, elem, hit, stats"""
    S = HI.soup()
    xyz, q, hausd = HI.frame_inputs(fi)
    met = None if metric is None else S["sol"][metric]
    fs = [S["sol"][f] for f in fields]
    sizes = ([met.shape[1]] if met is not None else []) + [f.shape[1] for f in fs]
    packed = form != "arrays"
    env = {"PMMG_HIP_PACKPASS": form[-1]} if packed else None
    ctx = make_ctx(sort, env)
    try:
        n = q.shape[0]
        adja = np.zeros((S["tetv"].shape[0], 4), np.int32)
        ctx.set_background_tet8(ctx.upload(xyz), ctx.upload(pack_tet8(S["tetv"], adja)), ctx.upload(S["triv"]),
                                ctx.upload(np.zeros((S["triv"].shape[0], 3), np.int32)), hausd)
        if packed:
            ctx.set_solutions_packed(ctx.upload(pack_solutions(met, fs)), 0 if met is None else met.shape[1],
                                     [f.shape[1] for f in fs])
        else:
            ctx.set_solutions(None if met is None else ctx.upload(met), [ctx.upload(f) for f in fs])
        if route != "nomap":
            ctx.set_point_map(ctx.upload(S["src"] if route == "map" else S["far"]))
        el, hit = ctx.upload(np.zeros(n, np.int32)), ctx.upload(np.zeros(n, np.int8))
        dq, dpc = ctx.upload(q), ctx.upload(S["pclass"])
        if form.startswith("rec"):
            rs = (sum(sizes) + 1) & ~1
            ro = ctx.upload(np.full((n, rs), SENT))
            st = ctx.locate_interp_rec(dq, dpc, ro, el, hit)
            r, rows, o = ro.download(), [], 0
            for s in sizes:
                rows.append(np.ascontiguousarray(r[:, o:o + s]))
                o += s
            assert (r[:, o:].view(np.uint64) == SENT_BITS).all(), "the records' padding was written"
        else:
            outs = [ctx.upload(np.full((n, s), SENT)) for s in sizes]
            st = ctx.locate_interp(dq, dpc, outs[0] if met is not None else None,
                                   outs[1:] if met is not None else outs, el, hit)
            rows = [o.download() for o in outs]
        names = ([metric] if metric else []) + list(fields)
        return dict(rows=rows, names=names, elem=el.download(), hit=hit.download(), stats=st.as_dict())
    finally:
        ctx.close()


def check_soup(fi, out, metric, route, what):
    """elem and hit as the route demands, then every row within its bound; prints the worst error/bound per class"""
    S = HI.soup()
    ref = HI.reference(fi)
    code, loc = out["hit"].astype(np.int32) & 15, (out["hit"].astype(np.int32) >> 4) & 3
    worst = {}
    nmap_v = nmap_b = 0
    for i, r in enumerate(ref):
        h, vol = int(code[i]), S["pclass"][i] == 1
        assert out["elem"][i] == S["own"][i], (what, i, S["label"][i], out["elem"][i], S["own"][i], h)
        accepted = r["phimin"] > -HI.MMG_EPS
        if vol:
            nmap_v += 1
            if not accepted:
                assert h == HI.VOL_CLOSEST, (what, i, h)
            elif route == "map":
                assert h == HI.VOL_WALK, (what, i, h)
            elif route == "far":
                assert h == HI.VOL_EXHAUST, (what, i, h)
            else:
                assert h in (HI.VOL_WALK, HI.VOL_EXHAUST), (what, i, h)
        else:
            nmap_b += 1
            own_kind = (r["kind"], r["loc"] if r["kind"] != HI.BDY_FACE else 0)
            if route == "map":
                assert (h, int(loc[i])) == own_kind, (what, i, h, loc[i], own_kind)
            elif route == "far":
                assert h == HI.BDY_EXHAUST, (what, i, h)
            else:
                assert h == HI.BDY_EXHAUST or (h, int(loc[i])) == own_kind, (what, i, h, loc[i], own_kind)
        want = HI.rule_rows(r, h, metric)
        for name, rows in zip(out["names"], out["rows"]):
            val, bnd = want[name]
            if val is None:
                assert (rows[i].view(np.uint64) == SENT_BITS).all(), (what, i, name, "a failed inversion's row was written")
                continue
            assert not (rows[i].view(np.uint64) == SENT_BITS).any(), (what, i, name, "row not written")
            ratio, _ = HI.row_ratio(rows[i], val, bnd)
            cls = "p1" if name in HI.ISO else (S["tet_class"] if vol else S["tri_class"])[S["own"][i] - 1][
                0 if name == "met6" else 1]
            worst[cls] = max(worst.get(cls, 0.0), ratio)
            assert ratio <= 1.0, (what, i, S["label"][i], h, name, ratio, rows[i], [float(v) for v in val])
    if route != "nomap":
        assert out["stats"]["nvol_src"] == nmap_v and out["stats"]["nbdy_src"] == nmap_b, out["stats"]
    else:
        assert out["stats"]["nvol_src"] == 0 and out["stats"]["nbdy_src"] == 0
    print(what, "worst error/bound", {k: round(v, 3) for k, v in sorted(worst.items())},
          "hits", np.bincount(code, minlength=12).tolist())


@pytest.mark.gpu
@pytest.mark.parametrize("sort", [False, True], ids=["input", "morton"])
@pytest.mark.parametrize("route", ["map", "far", "nomap"])
@pytest.mark.parametrize("fi", range(len(HI.FRAMES)))
def test_rows_within_bounds_in_every_frame(fi, route, sort):
    """(6, 1, 3, 6) and the iso metric's (1, 1, 1) in each frame, by each route, in both query orders"""
    for layout in ((6, 1, 3, 6), (1, 1, 1)):
        metric, fields = names_of(layout)
        out = run_soup(fi, metric, fields, "arrays", route, sort)
        check_soup(fi, out, metric, route, f"frame {fi} {route} {'morton' if sort else 'input'} {layout}")


def _same(a, b):
    np.testing.assert_array_equal(a["elem"], b["elem"])
    np.testing.assert_array_equal(a["hit"], b["hit"])
    for x, y in zip(a["rows"], b["rows"]):
        assert np.array_equal(x.view(np.uint64), y.view(np.uint64))


@pytest.mark.gpu
@pytest.mark.parametrize("layout", LAYOUTS + (RUNTIME,), ids=lambda l: "-".join(map(str, l)) or "none")
def test_every_layout_in_every_form(layout):
    """each compiled layout and the runtime one, on the unit frame: arrays, packed
    records in one and two passes and output records where the form exists, with
    the map, against it and without one (the plain kernels, k_vol<..., 0> and
    k_bdy<0>: the seed grid finds most trias and some tetra by itself, the
    exhaustive searches the rest), in input and Morton order; the forms of one
    layout bit-identical to each other"""
    metric, fields = names_of(layout, metric=layout != RUNTIME)
    passes = () if layout == RUNTIME else packed_forms(layout)  # (packed records need a compiled layout)
    forms = ["arrays"] + [f"{kind}{p}" for p in passes for kind in ("packed", "rec")]
    for route in ("map", "far", "nomap"):
        for sort in (False, True):
            first = None
            for form in forms:
                out = run_soup(0, metric, fields, form, route, sort)
                if first is None:  # (the other forms must equal this one bit for bit: one comparison holds them all)
                    first = out
                    check_soup(0, out, metric, route, f"layout {layout} {form} {route} {'morton' if sort else 'input'}")
                else:
                    _same(first, out)
                    assert out["stats"]["nvol_src"] == first["stats"]["nvol_src"]
            if route == "nomap" and layout:  # the plain kernels' own interpolation ran, not the searches' alone
                code = first["hit"].astype(np.int32) & 15
                assert (code == HI.VOL_WALK).sum() > 0 and np.isin(code, (HI.BDY_FACE, HI.BDY_EDGE, HI.BDY_VERTEX)).sum() > 100
