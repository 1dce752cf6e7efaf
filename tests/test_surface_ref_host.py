"""The surface zoo of tests/surface_ref.py and the CPU oracle on it (CPU only;
the device is held to the same definition in test_gpu_surface.py).

Every condition the zoo is built for is computed here from the fixture itself;
the oracle alone must give the definition's answer to every query from three
different starts, none left out; and the altered definitions must differ from
the true one on the fixtures named for them."""
import numpy as np
import pytest

import highprec_interp as HI
import surface_ref as SR
from oracle import oracle as O

H = SR.HAUSD


@pytest.fixture(scope="module")
def Z():
    return SR.zoo()


def _pts(Z, k):
    return Z["xyz"][Z["triv"][k - 1] - 1]


def _normal(Z, k):
    a, b, c = _pts(Z, k)
    n = np.cross(b - a, c - a)
    return n / np.linalg.norm(n)


def _patches(Z, kind):
    return [p for p in Z["patch"] if p["kind"] == kind]


def _queries(Z, p=None, label=None):
    return [i for i in range(Z["q"].shape[0])
            if (p is None or Z["patch"][Z["qpatch"][i]] is p) and (label is None or Z["label"][i].startswith(label))]


def test_adjt_is_the_edge_dictionary(Z):
    """3 k + l on both sides of an edge of exactly two trias, 0 on every other edge; patches share nothing"""
    n2 = 0
    for (v, w), pair in Z["edges"].items():
        for i, (k, l) in enumerate(pair):
            assert {int(Z["triv"][k - 1][(l + 1) % 3]), int(Z["triv"][k - 1][(l + 2) % 3])} == {v, w}
            if len(pair) == 2:
                k2, l2 = pair[1 - i]
                assert Z["adjt"][k - 1, l] == 3 * k2 + l2
                n2 += 1
            else:
                assert Z["adjt"][k - 1, l] == 0
    assert n2 == int((Z["adjt"] != 0).sum()) > 0
    assert sorted(len(p) for p in Z["edges"].values())[-1] == 3  # the non-manifold edge, and nothing above it
    for p in Z["patch"]:
        assert set(Z["triv"][p["t0"] - 1:p["t1"] - 1].ravel()) <= set(range(p["v0"], p["v1"]))
        lo = Z["xyz"][p["v0"] - 1:p["v1"] - 1]
        assert np.abs(lo - p["origin"]).max() < 0.45 * SR.SPACING  # apart by more than a tenth of the spacing
    assert Z["tetv"].shape == (1, 4) and (Z["pclass"] == 2).all()
    assert (Z["lowest"][Z["src"] - 1] == Z["starts"][:, 0]).all()
    for qi in range(Z["q"].shape[0]):
        assert set(Z["starts"][qi]) <= Z["home"][qi] and len(set(Z["starts"][qi])) == 3


def test_ridges_are_what_they_claim(Z):
    """each dihedral angle, measured on the side the normals leave; the shared edge at local index 0, 1 and 2 of
    either tria; generic coordinates and edge lengths; the queries at their distances from the edge line"""
    seen_a, seen_b, lengths = set(), set(), set()
    for p, theta in zip(_patches(Z, "ridge"), SR.RIDGE_ANGLES):
        assert p["theta"] == theta
        a1, b1 = p["t0"], p["t0"] + 1
        e = (p["v0"], p["v0"] + 1)
        pair = dict(Z["edges"][e])
        assert set(pair) == {a1, b1}
        seen_a.add(pair[a1]), seen_b.add(pair[b1])
        nA, nB = _normal(Z, a1), _normal(Z, b1)
        P, Q = Z["xyz"][e[0] - 1], Z["xyz"][e[1] - 1]
        RA = Z["xyz"][p["v0"] + 1]
        inA = (RA - P) - np.dot(RA - P, Q - P) / np.dot(Q - P, Q - P) * (Q - P)  # from the edge into A1
        between = np.degrees(np.arccos(np.clip(np.dot(nA, nB), -1, 1)))           # 180 - theta or theta - 180
        got = 180.0 - between if np.dot(nB, inA) < 0 else 180.0 + between         # convex: B's normal leaves A
        assert abs(got - theta) < 1e-6, (p["name"], got)
        lengths.add(round(float(np.linalg.norm(Q - P)), 6))
        assert np.abs(Q - P).min() > 0.01, "axis-aligned ridge"
        for r in (0.3, 0.7, 0.99, 1.01):
            (qi,) = _queries(Z, p, f"wedge-{r}")
            t, dist = SR._line(Z, Z["q"][qi], *e)
            assert abs(float(dist) / H - r) < 1e-9 and 0.2 < t < 0.8
        for label, side in (("alpha-below", -1), ("alpha-above", 1)):
            (qi,) = _queries(Z, p, label)
            t, dist = SR._line(Z, Z["q"][qi], *e)
            out = float(-t if side < 0 else t - 1) * np.linalg.norm(Q - P)  # how far the foot is past the end
            assert 0 < out < 0.05 * H and dist < H
        (qi,) = _queries(Z, p, "border")
        open_edge = (p["v0"], p["v0"] + 2)
        assert len(Z["edges"][open_edge]) == 1
        t, dist = SR._line(Z, Z["q"][qi], *open_edge)
        assert 0 < t < 1 and dist < H
    assert seen_a == seen_b == {0, 1, 2} and len(lengths) == len(SR.RIDGE_ANGLES)


def _apex_fan(Z, p):
    apex = p["v0"]
    return apex, Z["node_trias"][apex]


def test_fans_are_what_they_claim(Z):
    """each fan size around its apex, closed with open ring edges; which apexes the device has to scan for; the
    open fan's apex on the border; three sheets in one edge; two closed fans at the pinched vertices; stored
    orientations"""
    sizes = []
    for p in _patches(Z, "fan") + _patches(Z, "reject") + _patches(Z, "flipped"):
        apex, trias = _apex_fan(Z, p)
        n = p["n"]
        assert len(trias) == n == p["t1"] - p["t0"] and SR._fan_of(Z, apex, trias[0]) == set(trias)
        for k in trias:  # both spokes shared by two trias, the ring edge open
            l = list(Z["triv"][k - 1]).index(apex)
            assert Z["adjt"][k - 1, l] == 0 and (np.delete(Z["adjt"][k - 1], l) != 0).all()
        assert SR.scan_vertex(Z, apex) == (n > SR.FAN_MAX)
        ring = Z["xyz"][p["v0"]:p["v1"] - 1] - Z["xyz"][apex - 1]
        assert np.ptp(np.linalg.norm(ring, axis=1)) > (0.05 if n > 4 else 0.0)
        if p["kind"] == "fan" and p["name"] != "fan-exact":
            sizes.append(n)
    assert tuple(sizes) == SR.FAN_SIZES and {63, 64, 65, 66} <= set(sizes)
    (p,) = _patches(Z, "open")
    apex, trias = _apex_fan(Z, p)
    assert len(trias) == 5 and SR.scan_vertex(Z, apex)
    spokes = [e for e in Z["edges"] if apex in e]
    assert sorted(len(Z["edges"][e]) for e in spokes) == [1, 1, 2, 2, 2, 2]
    (p,) = _patches(Z, "nonmanifold")
    apex, trias = _apex_fan(Z, p)
    assert len(trias) == 9 and SR.scan_vertex(Z, apex) and len(p["comps"]) == 3
    assert len(Z["edges"][(apex, apex + 1)]) == 3
    for k, l in Z["edges"][(apex, apex + 1)]:
        assert Z["adjt"][k - 1, l] == 0
    for p in _patches(Z, "pinched"):
        apex, trias = _apex_fan(Z, p)
        assert len(trias) == sum(p["fans"]) and not SR.scan_vertex(Z, apex)  # every spoke has exactly two trias
        fans = sorted(len(c) for c in p["comps"])
        assert fans == sorted(p["fans"])
        for c in p["comps"]:
            assert SR._fan_of(Z, apex, min(c)) == set(c)  # a rotation from a tria closes on its own fan
            others = set().union(*[set(Z["triv"][k - 1]) for k in trias if k not in c])
            assert set().union(*[set(Z["triv"][k - 1]) for k in c]) & others == {apex}
    assert sorted(tuple(p["fans"]) for p in _patches(Z, "pinched")) == [(4, 4), (6, 3)]
    for p in _patches(Z, "flipped"):
        apex, trias = _apex_fan(Z, p)
        axis = p["R"] @ np.array([0.0, 0, 1.0])
        down = [i for i, k in enumerate(trias) if np.dot(_normal(Z, k), axis) < 0]
        assert tuple(down) == p["flip"] and 0 < len(down) < len(trias)


def test_one_rejecting_edge_at_every_position(Z):
    """in copy j the edge to ring vertex j alone makes an acute angle with the copy's queries; every position of
    the 12-fan and 0, 31, 62, 63 of the 64-fan occur"""
    seen = {12: [], 64: []}
    for p in _patches(Z, "reject"):
        apex, j = p["v0"], p["raised"]
        seen[p["n"]].append(j)
        qs = _queries(Z, p)
        assert len(qs) == 2
        for qi in qs:
            d = Z["q"][qi] - Z["xyz"][apex - 1]
            assert np.linalg.norm(d) < H
            ring = Z["xyz"][p["v0"]:p["v1"] - 1] - Z["xyz"][apex - 1]
            acute = np.nonzero(ring @ d > 0)[0]
            assert acute.tolist() == [j], (p["name"], acute)
            assert SR.define(Z, qi) == (SR.BDY_WEDGE, dict(Z["edges"][(apex, apex + 1 + j)]))
    assert tuple(seen[12]) == SR.REJECT12 and tuple(seen[64]) == SR.REJECT64


def test_queries_of_every_kind(Z):
    """no query is accepted by a tria, with a margin far above rounding; the cone queries at 0.5, 0.99 and 1.01
    hausd from their apex; the exact ones exactly hausd away in binary64; the kinds' counts"""
    kinds = []
    for qi in range(Z["q"].shape[0]):
        acc, margin = SR.accepting(Z, qi)
        assert not acc and margin > 1e-5, (qi, Z["label"][qi], acc, margin)
        kinds.append(SR.define(Z, qi)[0])
        p = Z["patch"][Z["qpatch"][qi]]
        lab = Z["label"][qi]
        if lab.startswith(("cone-0", "cone-1", "pinched-both")):
            r = float(lab.rsplit("-", 1)[1])
            assert abs(np.linalg.norm(Z["q"][qi] - Z["xyz"][p["v0"] - 1]) / H - r) < 1e-9
            assert kinds[-1] == (SR.BDY_CLOSEST if r > 1 else SR.BDY_WEDGE if p["kind"] == "reject" else SR.BDY_CONE)
    (qe,) = _queries(Z, None, "cone-exact")
    d = Z["q"][qe] - Z["xyz"][Z["patch"][Z["qpatch"][qe]]["v0"] - 1]
    assert np.sqrt(d[0] * d[0] + d[1] * d[1] + d[2] * d[2]) == H and kinds[qe] == SR.BDY_CONE
    (qw,) = _queries(Z, None, "wedge-exact")
    p = Z["patch"][Z["qpatch"][qw]]
    assert SR._line(Z, Z["q"][qw], p["v0"], p["v0"] + 1)[1] == H and kinds[qw] == SR.BDY_WEDGE
    count = np.bincount(kinds, minlength=12)
    print("definition's kinds: wedge %d cone %d closest %d of %d" % (count[7], count[8], count[11], len(kinds)))
    assert count[7] + count[8] + count[11] == len(kinds) and min(count[7], count[8], count[11]) >= 25
    for lab in ("alpha-below", "alpha-above"):
        assert all(kinds[qi] == SR.BDY_CONE for qi in _queries(Z, None, lab))
    assert all(kinds[qi] == SR.BDY_CLOSEST for qi in _queries(Z, None, "border") + _queries(Z, None, "pinched-one"))
    # the cone hits the device's rotation cannot finish: open ends of the ridges' patches, the open fan, the
    # three sheets, fans of 65 and 66 trias
    scans = [qi for qi in range(len(kinds)) if kinds[qi] == SR.BDY_CONE and SR.scan_vertex(Z, cone_vertex(Z, qi))]
    assert len(scans) >= 10 + 2 + 2 + 4


def cone_vertex(Z, qi):
    kind, elems = SR.define(Z, qi)
    assert kind == SR.BDY_CONE
    k, l = next(iter(elems.items()))
    return int(Z["triv"][k - 1][l])


def test_oracle_is_start_independent_and_equals_the_definition(Z):
    """O.run (MODE_FRESH) from three starts per query: the hit kind, the element set and loc are the
    definition's; runs that report the same tria give the same bits, those of O.eval_in_element; every row lies
    within the definition's bound.  No query is left out."""
    R = SR.oracle_from_starts()
    _, B = SR.background(Z)
    assert (R["anchor_elem"] == Z["starts"]).all(), "an anchor did not end in its tria"
    worst, elems_seen = {}, {7: set(), 8: set()}
    names = (SR.METRIC,) + SR.FIELDS
    for qi in range(Z["q"].shape[0]):
        kind, elems = SR.define(Z, qi)
        bits = {}
        for s in range(3):
            k, hit, loc = int(R["elem"][qi, s]), int(R["hit"][qi, s]), int(R["loc"][qi, s])
            what = (qi, Z["label"][qi], s, hit, k, loc)
            assert hit == kind and k in elems, (what, kind, sorted(elems))
            if kind in (SR.BDY_WEDGE, SR.BDY_CONE):
                assert loc == elems[k], (what, elems[k])
                elems_seen[kind].add((qi, k))
            got = [R["met"][qi, s]] + [f[qi, s] for f in R["fields"]]
            row = np.concatenate(got).view(np.uint64).tolist()
            assert bits.setdefault(k, row) == row, (what, "two starts, one tria, different bits")
            met, fr = O.eval_in_element(B, Z["q"][qi], True, k, hit, max(loc, 0))
            assert np.concatenate([met] + fr).view(np.uint64).tolist() == row, what
            want = SR.rows(qi, kind, k, elems[k])
            for name, g in zip(names, got):
                ratio, _ = HI.row_ratio(g, *want[name])
                key = (kind, "p1" if SR.SIZE[name] < 6 else "tensor")
                worst[key] = max(worst.get(key, 0.0), ratio)
                assert ratio <= 1.0, (what, name, ratio)
            if kind == SR.BDY_CONE:  # the vertex's metric row, bit for bit
                v = int(Z["triv"][k - 1][loc])
                assert np.array_equal(got[0].view(np.uint64), Z["sol"][SR.METRIC][v - 1].view(np.uint64)), what
    print("oracle worst error/bound", {f"{k[0]}-{k[1]}": round(v, 3) for k, v in sorted(worst.items())},
          "distinct (query, tria) reported: wedge %d cone %d" % (len(elems_seen[7]), len(elems_seen[8])))
    assert 0 < max(worst.values()) <= 1.0


def test_altered_definitions_differ_where_they_should(Z):
    """the fan by rotation from the walk's tria: a cone at the pinched vertices where one fan alone admits the
    point, and nowhere else (this is the device's documented deviation: device_define); distances tested with
    <: the two queries exactly hausd away; the ends exchanged: every query past an end of its edge"""
    nq = Z["q"].shape[0]
    true = [SR.define(Z, qi) for qi in range(nq)]
    rot = [qi for qi in range(nq) if SR.define(Z, qi, fan="rotation") != true[qi]]
    assert rot == _queries(Z, None, "pinched-one-fan") and len(rot) == 6
    for qi in rot:
        kind, elems = SR.device_define(Z, qi)
        apex = Z["patch"][Z["qpatch"][qi]]["v0"]
        assert kind == SR.BDY_CONE and true[qi][0] == SR.BDY_CLOSEST and set(elems) == set(Z["node_trias"][apex])
        # the rejecting trias all lie outside the home fan
        assert SR.in_cone(Z, Z["q"][qi], apex, Z["home"][qi])
        assert not SR.in_cone(Z, Z["q"][qi], apex, set(Z["node_trias"][apex]) - Z["home"][qi])
    strict = [qi for qi in range(nq) if SR.define(Z, qi, strict=True) != true[qi]]
    assert strict == _queries(Z, None, "wedge-exact") + _queries(Z, None, "cone-exact")
    assert all(SR.define(Z, qi, strict=True)[0] == SR.BDY_CLOSEST for qi in strict)
    swapped = [qi for qi in range(nq) if SR.define(Z, qi, swap_ends=True) != true[qi]]
    assert set(_queries(Z, None, "alpha-")) <= set(swapped)
    assert swapped == [qi for qi in range(nq) if true[qi][0] == SR.BDY_CONE]
    assert all(SR.define(Z, qi, swap_ends=True)[0] == SR.BDY_CLOSEST for qi in swapped)
    # the wedge's weights with the ends exchanged fall outside the bounds
    (qi,) = _queries(Z, Z["patch"][0], "wedge-0.3")
    k, l = next(iter(true[qi][1].items()))
    p = _pts(Z, k)
    (w0, w1), (d0, d1) = SR.wedge_weights(p[(l + 1) % 3], p[(l + 2) % 3], Z["q"][qi])
    assert abs(w0 - w1) > 1e6 * (d0 + d1)
