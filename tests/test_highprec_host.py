"""The CPU oracle's quality and weight arithmetic against the 50-digit
restatement of tests/highprec.py (CPU only; the device is held to the same
bounds in test_gpu_quality.py and test_gpu_wgt.py).

The oracle (oracle/pmmg_oracle.c) and the kernels (pmmg_quality.hip /.hpp)
share one text, so the bit-for-bit tests cannot see a formula or a table that
is wrong in both.  Here every element of the seeded inputs must lie within its
own forward error bound of the mathematical value, a high share of the bounds
must be tight (below 1e-9 relative: a bound that lets everything through fails),
and deliberately altered formulas must fall outside the bounds.

Worst |oracle - value| / bound measured on these inputs (printed by each test):
qual_iso 0.29, qual_ani 0.16, iso weight 0.48, aniso weight 0.15.  (The oracle
exposes no edge length; the device's length list is held to len_iso / len_ani
in test_gpu_wgt.py: 0.45 and 0.21.)"""
import numpy as np
import pytest

import highprec as H
from oracle import oracle as O
from parmmg_amd import synth

mp = H.mp

# the shares of tight bounds (bound < 1e-9 |value|) required below: the 1e-7 and
# 1e-9 slivers (240 + 120 of 1860 tetra) cannot have one, nor can a tensor whose
# determinant cancels over an eigenvalue ratio near 1e8; measured 0.806 (iso
# quality), 0.582 (aniso quality), 1.0 (weights), required just below that
TIGHT = dict(qual_iso=0.8, qual_ani=0.55, wgt_iso=0.95, wgt_ani=0.95)


def _report(name, rat, tight):
    print(f"{name}: n {rat.size} worst error/bound {rat.max():.3g} tight share {tight:.3f}")


@pytest.mark.parametrize("ani", [False, True], ids=["iso", "ani"])
def test_oracle_quality_within_bounds(ani):
    xyz, tetv, labels = H.qual_geometry()
    assert tetv.shape[0] <= 2000 and {"regular", "normal", "sliver1e-03", "sliver1e-07", "sliver1e-09"} == set(labels)
    met = H.qual_tensors() if ani else None
    val, bnd = H.qual_reference(ani)
    got, _ = O.tetra_qual(xyz, tetv, met)
    assert (got > 0).all(), "every tetra of the inputs is positively oriented"
    rat, tight = H.ratios(got, val, bnd)
    _report("qual_ani" if ani else "qual_iso", rat, tight)
    bad = np.nonzero(~(rat <= 1.0))[0]
    assert bad.size == 0, (bad[:5], [labels[i] for i in bad[:5]], rat[bad[:5]])
    assert tight >= TIGHT["qual_ani" if ani else "qual_iso"]
    # a regular tetra scores 1 / ALPHAD in any frame, in any metric c I
    reg = [i for i, l in enumerate(labels) if l == "regular"]
    if not ani:
        assert all(abs(val[i] * mp.mpf(12) * mp.sqrt(3) - 1) < 1e-9 for i in reg)


def _oracle_faces(xyz, tetv, met):
    return np.array([[O.face_wgt(xyz, v, f, met) for f in range(4)] for v in tetv])


def test_iso_weight_inputs_cover_the_switch():
    xyz, tetv, met = H.wgt_iso_inputs()
    r = np.concatenate([H.iso_r(met, v) for v in tetv])
    a = np.abs(r)
    assert not ((a > 0.9e-6) & (a < 1.1e-6)).any()
    for s in (-1, 1):  # both signs on both sides, and h1 == h2
        assert ((a < 1e-6) & (a > 0) & (np.sign(r) == s)).sum() > 50 and ((a > 1e-6) & (np.sign(r) == s)).sum() > 50
    for target in H.R_SWITCH:
        assert (np.abs(a - target) < 1e-3 * target).sum() >= 10, target
    assert (met >= 0.3 * (1 - 2e-3)).all() and (met <= 1.5 * (1 + 2e-3)).all()


def test_oracle_iso_weights_within_bounds():
    xyz, tetv, met = H.wgt_iso_inputs()
    assert 4 * tetv.shape[0] <= 2000
    val, bnd, _ = H.wgt_reference(False)
    got = _oracle_faces(xyz, tetv, met)
    rat, tight = H.ratios(got.ravel(), H.flat(val), H.flat(bnd))
    _report("wgt_iso", rat, tight)
    assert (rat <= 1.0).all(), np.nonzero(~(rat <= 1.0))[0][:5]
    assert tight >= TIGHT["wgt_iso"]
    assert (got == 1e6).sum() > 50 and (got < 1e6).sum() > 500  # below and at the cap


def test_oracle_aniso_weights_within_bounds_and_none_ambiguous():
    xyz, tetv, met = H.wgt_ani_inputs()
    assert 4 * tetv.shape[0] <= 2000
    gaps = np.concatenate([H.ani_gaps(xyz, met, v) for v in tetv])
    assert not ((gaps > 0.049) & (gaps < 0.051)).any()
    assert (gaps <= 0.049).sum() > 500 and (gaps >= 0.051).sum() > 500  # both branches
    val, bnd, amb = H.wgt_reference(True)
    assert sum(H.flat(amb)) == 0, "an edge of the inputs sits on the 0.05 switch"
    got = _oracle_faces(xyz, tetv, met)
    rat, tight = H.ratios(got.ravel(), H.flat(val), H.flat(bnd))
    _report("wgt_ani", rat, tight)
    assert (rat <= 1.0).all(), np.nonzero(~(rat <= 1.0))[0][:5]
    assert tight >= TIGHT["wgt_ani"]
    assert (got == 1e6).sum() > 50 and (got < 1e6).sum() > 500
    # edge lengths on both sides of 1
    lens = [float(H.len_ani(xyz[a - 1], xyz[b - 1], met[a - 1], met[b - 1])[0])
            for v in tetv[:60] for a, b in H.face_edges(v, 0)]
    assert min(lens) < 0.8 and max(lens) > 1.25


def test_weight_of_unit_lengths_is_exactly_one():
    """unit edges in the unit metric: res = 0 and the weight is 1, in mpmath as in the oracle"""
    v = np.array([1, 2, 3, 4], np.int32)
    reg = H.REG / np.sqrt(8.0)  # every edge sqrt(8) / sqrt(8): 1 up to the rounding of the coordinates
    for met in (np.ones((4, 1)), np.tile([1.0, 0, 0, 1.0, 0, 1.0], (4, 1))):
        for f in range(4):
            w, b, _ = H.face_wgt(reg, v, f, met)
            assert abs(w - 1) <= mp.mpf(1e-14)
            assert abs(mp.mpf(O.face_wgt(reg, v, f, met)) - w) <= b


SWAPPED = (H.IARF[0], H.IARF[2], H.IARF[1], H.IARF[3])  # rows 1 and 2 exchanged


@pytest.mark.parametrize("name,kw,ani", [("iarf-rows-swapped", dict(iarf=SWAPPED), False),
                                         ("28/3-is-9", dict(rate=(9, 1)), False),
                                         ("simpson-4-is-2", dict(simpson=2), True)])
def test_bounds_catch_an_altered_formula(name, kw, ani):
    """The harness' own check (no kernel runs): the oracle held to an altered
    mpmath variant falls outside the bound on at least 90 % of the generic cases
    — the faces the alteration touches, below the cap, and for Simpson's weight
    the faces with an edge in that branch."""
    xyz, tetv, met = H.wgt_ani_inputs() if ani else H.wgt_iso_inputs()
    _, bnd, _ = H.wgt_reference(ani)
    idx = range(1, tetv.shape[0], 4)  # 105 tetra (odd ones: the aniso inputs' Simpson half)
    missed = total = 0
    for k in idx:
        v = tetv[k]
        if ani and (H.ani_gaps(xyz, met, v) < 0.05).all():
            continue
        for f in ((1, 2) if "iarf" in kw else range(4)):
            if ani and (H.ani_gaps(xyz, met, v)[list(H.IARF[f])] < 0.05).all():
                continue
            got = O.face_wgt(xyz, v, f, met)
            w, _, _ = H.face_wgt(xyz, v, f, met, **kw)
            if got == 1e6 and w >= 1e6:
                continue  # both capped: the alteration cannot show
            total += 1
            missed += int(abs(mp.mpf(got) - w) <= bnd[k][f])
    print(name, "generic cases", total, "not caught", missed)
    assert total >= 60
    assert missed <= 0.1 * total


def _lattice():
    m = synth.lattice(synth.CUBE, 5, jitter=0.15, seed=5)
    return m, H.graded_sizes(m.xyz), H.stretched_metric(m.xyz)


def lattice_metric(kind):
    """(mesh, metric): "iso", "aniso" (the 1e4 stretch) or "aniso-mild" (lengths near 1: weights below the cap)"""
    m, iso, ani = _lattice()
    if kind == "aniso-mild":
        return m, H.stretched_metric(m.xyz, (0.6, 1.0, 1.8))
    return m, dict(iso=iso, aniso=ani)[kind]


def test_lengths_within_bounds_on_the_lattice():
    """The oracle exposes no edge length, so len_iso / len_ani are pinned by
    known answers: a constant size h gives l / h, a size ratio of 2 gives l ln 2
    / h1, a constant tensor gives sqrt(e^T M e), tensors M and 4 M give (1 + 2 + 4
    sqrt 2.5) / 6 of it; and no edge of the lattice the GPU test measures sits on
    a switch."""
    a, b = np.array([0.1, 0.2, 0.3]), np.array([0.9, -0.4, 0.5])
    l = mp.sqrt(sum((mp.mpf(float(y)) - mp.mpf(float(x))) ** 2 for x, y in zip(a, b)))
    v, bd = H.len_iso(a, b, 0.7, 0.7)
    assert abs(v - l / mp.mpf(0.7)) < 1e-40 and bd < 1e-15 * v
    v, bd = H.len_iso(a, b, 0.5, 1.0)
    assert abs(v - l * mp.log(2) / mp.mpf(0.5)) < 1e-40
    s = np.array([2.0, 0.3, -0.1, 1.5, 0.2, 3.0])
    v, bd, amb = H.len_ani(a, b, s, s)
    e = b - a
    M = np.array([[s[0], s[1], s[2]], [s[1], s[3], s[4]], [s[2], s[4], s[5]]])
    assert abs(float(v) - np.sqrt(e @ M @ e)) < 1e-14 and not amb
    v2, _, _ = H.len_ani(a, b, s, 4 * s)  # Simpson of a linear sqrt: (1 + 2 + 4 sqrt(2.5)) / 6 of it
    assert abs(v2 / v - (3 + 4 * mp.sqrt(mp.mpf(2.5))) / 6) < 1e-40
    m, iso, ani = _lattice()
    edges = sorted({(int(min(t[i], t[j])), int(max(t[i], t[j]))) for t in m.tetv for i, j in H.IARE})
    amb = sum(int(H.len_ani(m.xyz[p - 1], m.xyz[q - 1], ani[p - 1], ani[q - 1])[2]) for p, q in edges)
    assert amb == 0
    r = np.abs(np.array([iso[q - 1, 0] / iso[p - 1, 0] - 1.0 for p, q in edges]))
    assert not ((r > 0.9e-6) & (r < 1.1e-6)).any()


def graph_weight_check(m, met, wgt_of):
    """(skipped, total) over the interior faces of m: wgt_of(k, f) must equal
    max((int) w, 1) of the mpmath weight; an entry is skipped only where floor(w
    - bound) and floor(w + bound) differ."""
    skipped = total = 0
    for k in range(m.ne):
        for f in range(4):
            if not m.adja[k, f]:
                continue
            w, b, _ = H.face_wgt(m.xyz, m.tetv[k], f, met)
            total += 1
            if mp.floor(w - b) != mp.floor(w + b):
                skipped += 1
                continue
            assert wgt_of(k, f) == max(int(mp.floor(w)), 1), (k, f, w, wgt_of(k, f))
    return skipped, total


@pytest.mark.parametrize("kind", ["iso", "aniso", "aniso-mild"])
def test_graph_weight_restatement_within_bounds(kind):
    """max((int) w, 1) of the oracle's weight, as tests/test_metis_graph.py
    restates the graph's weights, agrees with mpmath's on the 5^3 lattice and
    skips fewer than 1 % of the entries"""
    m, met = lattice_metric(kind)
    w = {}

    def oracle_weight(k, f):
        w[(k, f)] = O.face_wgt(m.xyz, m.tetv[k], f, met)
        return max(int(w[(k, f)]), 1)

    skipped, total = graph_weight_check(m, met, oracle_weight)
    free = sum(1 for x in w.values() if x < 1e6)
    print(kind, "entries", total, "skipped", skipped, "below the cap", free)
    assert total > 1000 and skipped < 0.01 * total
    assert free == 0 if kind == "aniso" else free > 0.5 * total  # (the 1e4 stretch caps every weight)
