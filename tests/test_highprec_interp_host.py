"""The CPU oracle's interpolation against the 50-digit restatement of
tests/highprec_interp.py (CPU only; the device is held to the same bounds in
test_gpu_interp_highprec.py).

parity.check compares the device's rows with O.eval_in_element, a restatement
in the kernels' own operation order by the same hands: a formula wrong in both
passes.  Here every row the oracle gives for the soup's queries, in three
frames, must lie within its own forward error bound of the value of the
definition, a stated share of the bounds must be tight, the inputs must be what
they claim to be, and altered definitions must fall outside the bounds."""
import functools

import numpy as np
import pytest

import highprec as H
import highprec_interp as HI
from oracle import oracle as O

mp = H.mp
FIELDS6 = ("ten6", "s0", "s1", "s2", "s3", "s4", "vec")
NFRAMES = len(HI.FRAMES)

# The shares of tight rows (every bound of the row below 1e-9 of its largest
# modulus) required below, per class, over the three frames: measured
# MEASURED_TIGHT, required just below that.  In frames 0 and 2 alone the shares are
# 0.99 (p1), 0.96 to 0.99 (the tensor classes) and 0.85 (stretch-1e4).  What cannot
# be tight: the 1e-5 slivers, whose coordinates carry 8 u perm / |D| of about 1e-9
# in the unit frame already (a sixth of the tetra); frame 1, where the coordinates'
# spacing (1e-13 beside elements of 3e-5) is the projected point's error on every
# tria (shares of 0.62 to 0.76 there); a stretch of 1e4 twice inverted, whose bound
# reaches 1e-8 of the row.
MEASURED_TIGHT = {"p1": 0.923, "same-rotation": 0.880, "rotation-per-vertex": 0.887, "stretch-1e2": 0.876,
                  "stretch-1e4": 0.770, "shortcut-input": 0.889, "shortcut-mint": 0.913}
TIGHT = {"p1": 0.91, "same-rotation": 0.87, "rotation-per-vertex": 0.87, "stretch-1e2": 0.86,
         "stretch-1e4": 0.76, "shortcut-input": 0.87, "shortcut-mint": 0.90}
# The same shares in frames 0 and 2 without the 1e-5 slivers, which is the derivation's own tightness: measured 1.000
# for every class but stretch-1e4 at 0.899, whose bound is the condition of a 1e4 stretch inverted twice (u * 1e4 on
# the first inverses, times 1e4 again: up to 1e-8 of the row); required just below
TIGHT_DERIVATION = {"p1": 0.995, "same-rotation": 0.995, "rotation-per-vertex": 0.995, "stretch-1e2": 0.995,
                    "stretch-1e4": 0.88, "shortcut-input": 0.995, "shortcut-mint": 0.995}
# worst |oracle - value| / bound measured per class over the three frames (printed by test_oracle_within_bounds)
MEASURED_WORST = {"p1": 0.41, "same-rotation": 0.072, "rotation-per-vertex": 0.20, "stretch-1e2": 0.34,
                  "stretch-1e4": 0.22, "shortcut-input": 0.30, "shortcut-mint": 0.30}


def _class_of(S, i, name):
    """the class a row is reported under: p1 for the linear rows, the element's tensor class else"""
    if name in HI.ISO:
        return "p1"
    cls = (S["tet_class"] if S["pclass"][i] == 1 else S["tri_class"])[S["own"][i] - 1]
    return cls[HI.TENSOR.index(name)]


@functools.lru_cache(maxsize=None)
def oracle_rows(fi):
    """per query {rule: {solution: row}} as O.eval_in_element gives them in the
    query's own element, for the rules of HI.reference"""
    S = HI.soup()
    _, q, _ = HI.frame_inputs(fi)
    ref = HI.reference(fi)
    _, B6 = HI.background(fi, "met6", FIELDS6)
    _, B1 = HI.background(fi, "met1")
    out = []
    for i in range(q.shape[0]):
        bdy = S["pclass"][i] == 2
        k = int(S["own"][i])
        rules = dict(all=(9, 0), met=(ref[i]["kind"], ref[i]["loc"])) if bdy else dict(all=(2, 0), closest=(3, 0))
        rows = {}
        for rule, (hit, loc) in rules.items():
            m6, f = O.eval_in_element(B6, q[i], bdy, k, hit, loc)
            m1, _ = O.eval_in_element(B1, q[i], bdy, k, hit, loc)
            r = dict(met6=m6, met1=m1)
            if rule != "met":
                r.update(zip(FIELDS6, f))
            rows[rule] = r
        out.append(rows)
    return out


def _table(fi):
    """[(query, rule, solution, class, ratio, tight)] of frame fi; a row the
    definition leaves untouched must be untouched (NaN) in the oracle: ratio 0"""
    S = HI.soup()
    ref, got = HI.reference(fi), oracle_rows(fi)
    tab = []
    for i, (r, g) in enumerate(zip(ref, got)):
        for rule, rows in g.items():
            for name, row in rows.items():
                val, bnd = r[rule][name]
                if val is None:
                    assert np.isnan(row).all(), (fi, i, rule, name, row)
                    continue
                assert not np.isnan(row).any(), (fi, i, rule, name, "the oracle left a row the definition writes")
                ratio, tight = HI.row_ratio(row, val, bnd)
                tab.append((i, rule, name, _class_of(S, i, name), ratio, tight))
    return tab


@pytest.mark.parametrize("fi", range(NFRAMES))
def test_oracle_within_bounds(fi):
    tab = _table(fi)
    S = HI.soup()
    for cls in ("p1",) + HI.TENSOR_CLASSES:
        rows = [t for t in tab if t[3] == cls]
        worst = max(rows, key=lambda t: t[4])
        print(f"frame {fi} {cls}: rows {len(rows)} worst error/bound {worst[4]:.3g} "
              f"(query {worst[0]} {S['label'][worst[0]]} {worst[1]} {worst[2]}) "
              f"tight share {sum(t[5] for t in rows) / len(rows):.3f}")
    bad = [t for t in tab if not t[4] <= 1.0]
    assert not bad, bad[:5]


def test_tight_shares():
    tab = [t for fi in range(NFRAMES) for t in _table(fi)]
    for cls in ("p1",) + HI.TENSOR_CLASSES:
        rows = [t for t in tab if t[3] == cls]
        share = sum(t[5] for t in rows) / len(rows)
        print(f"{cls}: tight share {share:.3f} of {len(rows)} rows")
        assert share >= TIGHT[cls], (cls, share)
    # the derivation itself: the same shares without what the inputs make loose (frame 1, the 1e-5 slivers)
    S = HI.soup()
    tab = [t for fi in (0, 2) for t in _table(fi)
           if S["pclass"][t[0]] == 2 or S["tet_kind"][S["own"][t[0]] - 1] != "sliver1e-05"]
    for cls in ("p1",) + HI.TENSOR_CLASSES:
        rows = [t for t in tab if t[3] == cls]
        share = sum(t[5] for t in rows) / len(rows)
        print(f"{cls}: tight share {share:.3f} of {len(rows)} rows in frames 0 and 2 without the 1e-5 slivers")
        assert share >= TIGHT_DERIVATION[cls], (cls, share)


# ---------------------------------------------------------------- the inputs

def test_inputs_have_every_class():
    S = HI.soup()
    lab = np.array(S["label"])
    assert S["q"].shape[0] <= 2000
    for name in set(HI.TET_QUERY):
        assert (lab[S["pclass"] == 1] == name).sum() >= 100, name
    for name in set(HI.TRI_QUERY):
        assert (lab[S["pclass"] == 2] == name).sum() >= 90, name
    assert (lab == "outside").sum() == HI.N_OUTSIDE
    for kind in ("regular", "normal", "sliver1e-03", "sliver1e-05"):
        assert S["tet_kind"].count(kind) >= 25, kind
    for j in range(2):
        for cls in HI.TENSOR_CLASSES:
            assert sum(c[j] == cls for c in S["tet_class"]) >= 20 and sum(c[j] == cls for c in S["tri_class"]) >= 12
    # every tensor class meets every shape
    assert {(k, c[0]) for k, c in zip(S["tet_kind"], S["tet_class"]) if k != "binary"} == \
        {(k, c) for k in ("regular", "normal", "sliver1e-03", "sliver1e-05") for c in HI.TENSOR_CLASSES}
    dist = np.array([float(r["dist"]) for r in HI.reference(0)[S["nvol"]:]])
    assert (np.abs(dist) <= HI.HAUSD / 2).all() and (dist > 1e-4).sum() > 100 and (dist < -1e-4).sum() > 100
    s = S["sol"]
    assert all((s[n] > 0).any() and (s[n] < 0).any() for n in ("s0", "s1", "s2", "s4")) and (s["s3"] < 0).all()
    for name in HI.TENSOR:  # the stretches are what they are called: eigenvalues over 1 .. hi, a fifth past hi / 10
        for cls, hi in (("stretch-1e2", 1e2), ("stretch-1e4", 1e4)):
            j = HI.TENSOR.index(name)
            ids = np.concatenate([S["tetv"][k] for k, c in enumerate(S["tet_class"]) if c[j] == cls and
                                  S["tet_kind"][k] != "binary"])
            ratio = []
            for r in s[name][ids - 1]:
                lam = np.linalg.eigvalsh(np.array([[r[0], r[1], r[2]], [r[1], r[3], r[4]], [r[2], r[4], r[5]]]))
                assert lam[0] > 0.99 and lam[-1] < 1.01 * hi
                ratio.append(lam[-1] / lam[0])
            assert np.mean(np.array(ratio) > hi / 10) > 0.1 and max(ratio) > hi / 2


def test_the_shortcut_is_met_on_both_sides_and_nothing_sits_on_it():
    S = HI.soup()
    for name in HI.TENSOR:
        off = np.abs(S["sol"][name][:, [1, 2, 4]]).max(1)
        assert not ((off > 0.9e-6) & (off < 1.1e-6)).any()
        assert ((off < 0.9e-6) & (off > 0.3e-6)).sum() >= 40 and ((off > 1.1e-6) & (off < 2.1e-6)).sum() >= 40
    below = above = 0
    for fi in range(NFRAMES):
        for r in HI.reference(fi):
            for rule in ("all", "closest", "met"):
                for name in HI.TENSOR:
                    off = r.get(rule, {}).get("off:" + name)
                    if off is None:
                        continue
                    assert not 0.9e-6 < off < 1.1e-6, (fi, rule, name, off)
                    below += int(0.3e-6 < off < 0.9e-6)
                    above += int(1.1e-6 < off < 2.1e-6)
    print("interpolated inverses just below the switch", below, "just above", above)
    assert below >= 300 and above >= 300


@pytest.mark.parametrize("fi", range(NFRAMES))
def test_own_element_is_the_oracles(fi):
    """every accepted query's own element is the first that accepts it, every
    other volume query's own element is the closest, no coordinate sits on the
    acceptance threshold, and the surface hits' kinds are unambiguous"""
    S = HI.soup()
    _, q, hausd = HI.frame_inputs(fi)
    _, B = HI.background(fi)
    ref = HI.reference(fi)
    lab = S["label"]
    for i, r in enumerate(ref):
        assert abs(r["phimin"] + HI.MMG_EPS) > 1e-7, (i, r["phimin"])
        if S["pclass"][i] == 1:
            if r["phimin"] > -HI.MMG_EPS:
                assert O.first_accepting_tetra(B, q[i]) == S["own"][i], i
            else:
                assert O.first_accepting_tetra(B, q[i]) == 0 and O.closest_tetra(B, q[i]) == S["own"][i], i
            if lab[i] == "outside":
                assert -0.08 < r["phimin"] < -0.03
            elif fi != 1 and lab[i] != "fail":
                # -5e-7 as binary64 coordinates hold it: 1e-16 beside a 1e-5 sliver's height of 1e-6 is 1e-10 * 16;
                # (frame 1 rounds the coordinates by up to 1e-3 of such a height: its queries fall where they fall)
                assert r["phimin"] > -5.05e-7
        else:
            assert O.first_accepting_tria(B, q[i]) == S["own"][i], i
            assert abs(r["dist"]) <= hausd / 2 + r["ddist"]
            assert all(abs(p) <= 1e-8 or abs(p) >= 1e-3 for p in r["phi"]), (i, r["phi"])
            want = dict(face=HI.BDY_FACE, edge=HI.BDY_EDGE, vertex=HI.BDY_VERTEX).get(lab[i])
            assert want is None or r["kind"] == want, (i, lab[i], r["kind"])


def test_failure_routes_leave_rows_untouched():
    """in the frames whose coordinates are binary the designed failures fail, in the definition as in the oracle"""
    S = HI.soup()
    assert all(len(v) >= 1 for v in S["fail"].values())
    for fi in (0, 2):
        ref, got = HI.reference(fi), oracle_rows(fi)
        for key, idx in S["fail"].items():
            for i in idx:
                for name in HI.TENSOR:  # (the surface routes fail under the face rule and under the hit's own)
                    for rule in (("all",) if key.startswith("tet") else ("all", "met")):
                        if rule == "met" and name != "met6":
                            continue
                        assert ref[i][rule][name][0] is None, (fi, key, i, rule, name)
                        assert np.isnan(got[i][rule][name]).all()
                assert ref[i]["all"]["s1"][0] is not None and not np.isnan(got[i]["all"]["s1"]).any()


def test_affine_scalar_is_reproduced():
    """s0 is affine in x at the vertices, so its interpolant is the same function
    of the query, extrapolated points included, to within its bound and the
    rounding of the vertex values and of the frame's coordinates"""
    S = HI.soup()
    a = [mp.mpf(t) for t in HI.AFFINE]
    for fi in range(NFRAMES):
        s, t = (mp.mpf(x) for x in HI.FRAMES[fi])
        _, q, _ = HI.frame_inputs(fi)
        for i, r in enumerate(HI.reference(fi)):
            if S["pclass"][i] == 2:
                continue  # (off the plane of a tria the interpolant is the projection's value)
            x = [(mp.mpf(float(c)) - t) / s for c in q[i]]
            want = a[0] + sum(a[k + 1] * x[k] for k in range(3))
            val, bnd = r["all"]["s0"]
            # the vertex values are rounded sums of terms below 50 (4 u 50), and the frame's vertices sit within
            # u (|t| + 20 s) / s of the unit frame's in its units, times |a|_1 = 3.25, each weighted by |phi_i|
            slack = sum(abs(p) for p in r["phi"]) * H.U * (200 + mp.mpf("3.25") * 2 * (abs(t) + 20 * s) / s)
            assert abs(val[0] - want) <= bnd[0] + slack, (fi, i, val[0], want)


# ---------------------------------------------------------------- the harness' own check

def _generic(S, cls_ok, pclass, labels, n=120):
    """up to n queries of the unit frame of the given class with labels, whose met6 class passes cls_ok"""
    out = []
    for i in range(S["q"].shape[0]):
        if S["pclass"][i] != pclass or S["label"][i] not in labels:
            continue
        k = S["own"][i] - 1
        kind = S["tet_kind"][k] if pclass == 1 else "tria"
        if kind in ("sliver1e-05", "binary"):
            continue
        if cls_ok(_class_of(S, i, "met6")):
            out.append(i)
    return out[:n]


@pytest.mark.parametrize("variant", ["linear-in-M", "coordinates-exchanged", "edge-ends-l-l+1", "shortcut-ignored",
                                     "projection-omitted"])
def test_bounds_catch_an_altered_definition(variant):
    """The harness' own check (no kernel runs): the oracle held to an altered
    mpmath variant falls outside the bound on at least 90 % of the generic cases
    the alteration touches."""
    S = HI.soup()
    xyz, q, _ = HI.frame_inputs(0)
    ref, got = HI.reference(0), oracle_rows(0)
    sol = S["sol"]
    inv6 = HI.vertex_inverses("met6")
    smooth = lambda c: c in ("same-rotation", "rotation-per-vertex", "stretch-1e2")
    missed = total = 0

    def held(i, rule, name, val):
        nonlocal missed, total
        bnd = ref[i][rule][name][1]
        total += 1
        missed += int(HI.row_ratio(got[i][rule][name], val, bnd)[0] <= 1.0)

    if variant == "linear-in-M":
        for i in _generic(S, smooth, 1, ("interior", "c1e-3")):
            ids = S["tetv"][S["own"][i] - 1]
            held(i, "all", "met6", HI.interp_tensor(ref[i]["phi"], None, None, [sol["met6"][j - 1] for j in ids])[0])
    elif variant == "coordinates-exchanged":
        for i in _generic(S, lambda c: True, 1, ("interior", "c1e-3")):
            ids = [int(t) for t in S["tetv"][S["own"][i] - 1]]
            phi, dphi = HI.tet_coords(xyz[np.array(ids) - 1], q[i], exchange=(0, 1))
            held(i, "all", "vec", HI.interp_p1(phi, dphi, [sol["vec"][j - 1] for j in ids])[0])
    elif variant == "edge-ends-l-l+1":
        for i in _generic(S, smooth, 2, ("edge",)):
            ids = [int(t) for t in S["triv"][S["own"][i] - 1]]
            e = HI.edge_ends(ref[i]["loc"], altered=True)
            phi = [ref[i]["phi"][j] for j in e]
            held(i, "met", "met6", HI.interp_tensor(phi, [H.mp.mpf(0)] * 2, [inv6[ids[j] - 1] for j in e])[0])
            held(i, "met", "met1", HI.interp_p1(phi, [H.mp.mpf(0)] * 2, [sol["met1"][ids[j] - 1] for j in e])[0])
    elif variant == "shortcut-ignored":
        for i in _generic(S, lambda c: c.startswith("shortcut"), 1, ("interior", "c1e-3", "c0", "edge")) + \
                _generic(S, lambda c: c.startswith("shortcut"), 2, ("face",)):
            ids = S["tetv" if S["pclass"][i] == 1 else "triv"][S["own"][i] - 1]
            offs = [v[2] for v in (inv6[j - 1] for j in ids)] + [ref[i]["all"]["off:met6"]]
            if not any(0 < o < HI.MMG_EPS for o in offs):
                continue  # no inversion of this row takes the shortcut with something to drop
            full = [HI.invmat(HI._v(sol["met6"][j - 1]), shortcut=False) for j in ids]
            held(i, "all", "met6", HI.interp_tensor(ref[i]["phi"], ref[i]["dphi"], full, shortcut=False)[0])
    else:
        for i in _generic(S, lambda c: True, 2, ("face",)):
            if abs(ref[i]["dist"]) < 1e-4:
                continue
            ids = [int(t) for t in S["triv"][S["own"][i] - 1]]
            phi, dphi, _, _ = HI.tria_coords(xyz[np.array(ids) - 1], q[i], project=False)
            held(i, "all", "vec", HI.interp_p1(phi, dphi, [sol["vec"][j - 1] for j in ids])[0])
    print(variant, "generic cases", total, "not caught", missed)
    assert total >= 40
    assert missed <= 0.1 * total
