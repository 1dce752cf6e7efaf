"""pmmg_hip_compute_wgt_mesh / _faces (k_wgt_mesh, k_wgt_faces, pmmg_quality.hip;
face_wgt, lenedg_iso / _ani, wgt_term, wgt_of_res, pmmg_quality.hpp) on every
branch of the length and weight formulas, on the kernels' own semantics (which
entries they write, the tag mask, the face list), past the grid's cap, and
against the 50-digit reference of tests/highprec.py; and the two other routes
to the same arithmetic, the edge-length list and the METIS graph's weights,
under the same reference.

Contract, as in tests/test_wgt.py: 1e-13 relative to the oracle (the device's
exp / log1p are not the host's), NaN where the oracle has NaN; entries the
kernel must not write are compared as bytes.  Arrays sit behind
parity.device_view (tetv + 16, every other + 8, xt + 4) with their guard zones
checked after each call."""
import functools

import numpy as np
import pytest

import highprec as H
from oracle import oracle as O
from parity import device_view, make_ctx
from parmmg_amd import synth
from test_gpu_quality import TRIP, big_mesh, tiled
from test_highprec_host import _lattice, graph_weight_check, lattice_metric

pytestmark = pytest.mark.gpu

HUGE = 1.0e6
MG_PARBDY = 1 << 6
RTOL = 1e-13
SENT = np.array([0x7FF8C0DE0000F00D], np.uint64).view(np.float64)[0]
I6 = np.array([1.0, 0.0, 0.0, 1.0, 0.0, 1.0])


def close(got, want, what=""):
    """1e-13 relative, NaN where the oracle has NaN, infinities equal"""
    got, want = np.asarray(got), np.asarray(want)
    gn, wn = np.isnan(got), np.isnan(want)
    assert np.array_equal(gn, wn), (what, np.nonzero(gn != wn)[0][:8])
    np.testing.assert_allclose(got[~gn], want[~wn], rtol=RTOL, atol=0, err_msg=what)


class Views:
    """device_view of a set of arrays on one context; check() after a call:
    guards intact, inputs unchanged"""

    def __init__(self, ctx):
        self.ctx, self.v, self.al, self.src = ctx, {}, {}, {}

    def put(self, name, a, off, is_input=True):
        a = np.ascontiguousarray(a)
        self.v[name], self.al[name] = device_view(self.ctx, a, off)
        if is_input:
            self.src[name] = a
        return self.v[name]

    def check(self):
        for name, al in self.al.items():
            al.check(name)
        for name, a in self.src.items():
            assert np.array_equal(self.v[name].download().view(np.uint8), a.view(np.uint8)), f"{name} was written"

    def free(self):
        for al in self.al.values():
            al.free()
        self.v, self.al, self.src = {}, {}, {}


def run_mesh(ctx, xyz, tetv, xt, ftag, met, tag, qual0):
    vw = Views(ctx)
    try:
        d = [vw.put("xyz", xyz, 8), vw.put("tetv", np.asarray(tetv, np.int32), 16), vw.put("xt", np.asarray(xt, np.int32), 4),
             vw.put("ftag", np.asarray(ftag, np.uint16), 8)]
        dm = None if met is None else vw.put("met", met, 8)
        q = vw.put("qual", np.asarray(qual0, np.float64), 8, is_input=False)
        ctx.compute_wgt_mesh(d[0], d[1], d[2], d[3], dm, tag, q)
        out = q.download()
        vw.check()
        return out
    finally:
        vw.free()


def run_faces(ctx, xyz, tetv, face, met):
    face = np.ascontiguousarray(face, np.int32).reshape(-1, 2)
    vw = Views(ctx)
    try:
        d = [vw.put("xyz", xyz, 8), vw.put("tetv", np.asarray(tetv, np.int32), 16), vw.put("face", face, 8)]
        dm = None if met is None else vw.put("met", met, 8)
        w = vw.put("wgt", np.full(face.shape[0], SENT), 8, is_input=False)
        ctx.compute_wgt_faces(d[0], d[1], d[2], dm, w)
        out = w.download()
        vw.check()
        return out
    finally:
        vw.free()


def oracle_faces(xyz, tetv, met):
    """[ne, 4] oracle weights of every face, through the C loop: one face tagged at a time"""
    ne = tetv.shape[0]
    W = np.empty((ne, 4))
    for f in range(4):
        ftag = np.zeros((ne, 4), np.uint16)
        ftag[:, f] = 1
        W[:, f] = O.compute_wgt_mesh(xyz, tetv, np.ones(ne, np.int32), ftag, met, 1, np.zeros(ne))
    return W


def all_faces(ne):
    return np.array([(k + 1, f) for k in range(ne) for f in range(4)], np.int32)


# ---------------------------------------------------------------- branches

EQ = np.array([[0, 0, 0], [1, 1, 0], [1, 0, 1], [0, 1, 1]], np.float64)  # six edges of squared length 2, exactly
CORNER = np.array([[0, 0, 0], [1, 0, 0], [0, 1, 0], [0, 0, 1]], np.float64)
S2 = np.sqrt(2.0)
UNIT6 = np.array([1.0, 0.5, 0.5, 1.0, 0.5, 1.0])  # e^T M e = 1 for the six edges of CORNER, exactly


def _iso_cases():
    """name -> (vertices, sizes): one tetra each"""
    c = {}
    for name, r in (("r-under+", 0.5e-6), ("r-under-", -0.5e-6), ("r-over+", 2e-6), ("r-over-", -2e-6)):
        c[name] = (EQ, 0.8 * np.array([1.0, 1.0 + r, 1.0 + r, 1.0]))  # |r| on both sides of 1e-6, both signs
    c["h-equal"] = (EQ, np.full(4, 0.8))
    c["len-one-all"] = (EQ, np.full(4, S2))  # l = h = fl(sqrt 2) on every edge: len == 1, weight exactly 1
    c["len-one-x"] = (CORNER, np.ones(4))  # unit edges along the axes, h = 1: len == 1; the diagonals sqrt 2
    c["len-below-one"] = (EQ, np.full(4, S2 / 0.8))
    c["len-above-one"] = (EQ, np.full(4, S2 / 1.7))
    c["cap"] = (EQ, np.full(4, S2 / 0.5))  # res = -1.5: at the cap
    c["under-cap"] = (EQ, np.full(4, S2 / 0.507))  # res = -1.479: just under it
    c["short-edges"] = (EQ * 1e-9, np.full(4, 1.0))  # res = -3 (1 - 1e-9 per edge)
    c["h2-zero"] = (EQ, np.array([0.8, 0.8, 0.8, 0.0]))  # log1p(-1)
    c["h1-zero"] = (EQ, np.array([0.0, 0.8, 0.8, 0.8]))  # log1p(inf)
    return c


def _ani_cases():
    """name -> (vertices, [4, 6] tensors)"""
    ind = np.array([-1.0, 0.0, 0.0, -1.0, 0.0, 1.0])  # diag(-1, -1, 1): e^T M e <= 0 for the edges in the xy plane
    c = {}
    c["dd1-clamped"] = (CORNER, np.array([ind, I6, I6, I6]))  # edges 01, 02: dd1 = -1 -> 0, dd2 = 1
    c["dd2-clamped"] = (CORNER, np.array([I6, ind, ind, I6]))  # edges 01, 02: dd2 -> 0; edge 12: both
    c["dd-both-clamped"] = (CORNER, np.array([ind, ind, ind, ind]))
    c["gap-under"] = (CORNER, np.array([I6, 1.04 * I6, 1.04 * I6, I6]))  # |dd1 - dd2| = 0.04: midpoint
    c["gap-over"] = (CORNER, np.array([I6, 1.06 * I6, 1.06 * I6, I6]))  # 0.06: Simpson
    c["len-one-all"] = (CORNER, np.tile(UNIT6, (4, 1)))  # weight exactly 1
    c["len-below-one"] = (CORNER, np.tile(0.5 * UNIT6, (4, 1)))
    c["len-above-one"] = (CORNER, np.tile(3.0 * UNIT6, (4, 1)))
    c["cap"] = (CORNER, np.tile(0.25 * UNIT6, (4, 1)))  # len = 0.5 on every edge: res = -1.5
    c["under-cap"] = (CORNER, np.tile(0.507 ** 2 * UNIT6, (4, 1)))
    c["short-edges"] = (CORNER * 1e-9, np.tile(UNIT6, (4, 1)))
    c["graded"] = (CORNER, np.array([UNIT6, 2.0 * UNIT6, 0.5 * UNIT6, 4.0 * UNIT6]))
    return c


def _mesh_of(cases, width):
    xyz = np.vstack([p for p, _ in cases.values()])
    met = np.vstack([np.reshape(m, (4, width)) for _, m in cases.values()])
    tetv = np.arange(1, xyz.shape[0] + 1, dtype=np.int32).reshape(-1, 4)
    return np.ascontiguousarray(xyz), tetv, np.ascontiguousarray(met), {n: k for k, n in enumerate(cases)}


def test_iso_branches():
    xyz, tetv, met, at = _mesh_of(_iso_cases(), 1)
    ne = tetv.shape[0]
    # the branch each case is meant for, from the inputs alone
    r = {n: H.iso_r(met, tetv[k]) for n, k in at.items() if "zero" not in n}
    for n in ("r-under+", "r-under-"):  # (edges 01, 02 carry r, edges 13, 23 about -r: both signs either way)
        assert np.abs(r[n]).max() < 1e-6 and (r[n] > 0).sum() == 2 and (r[n] < 0).sum() == 2
    for n in ("r-over+", "r-over-"):
        assert (np.abs(r[n]) > 1e-6).sum() == 4 and (r[n] > 1e-6).sum() == 2 and (r[n] < -1e-6).sum() == 2
    assert not r["h-equal"].any()
    want = oracle_faces(xyz, tetv, met)
    ctx = make_ctx()
    try:
        got = run_faces(ctx, xyz, tetv, all_faces(ne), met).reshape(ne, 4)
        q = run_mesh(ctx, xyz, tetv, np.ones(ne, np.int32), np.full((ne, 4), 1, np.uint16), met, 1, np.zeros(ne))
        none = run_faces(ctx, xyz, tetv, all_faces(ne), None)
    finally:
        ctx.close()
    close(got, want, "iso faces")
    close(q, O.compute_wgt_mesh(xyz, tetv, np.ones(ne, np.int32), np.full((ne, 4), 1, np.uint16), met, 1, np.zeros(ne)),
          "iso mesh")
    assert (none == HUGE).all()  # met_size = 0
    assert (got[at["len-one-all"]] == 1.0).all()
    # len-one-x, face 3 (vertices 0 1 2): 1, 1 and sqrt 2 -> res = 1 / sqrt 2 - 1
    np.testing.assert_allclose(got[at["len-one-x"], 3], np.exp(-28.0 * (1 / S2 - 1) / 3.0), rtol=1e-13)
    np.testing.assert_allclose(got[at["len-below-one"]], np.exp(-28.0 * 3 * (0.8 - 1) / 3.0), rtol=1e-12)
    np.testing.assert_allclose(got[at["len-above-one"]], np.exp(-28.0 * 3 * (1 / 1.7 - 1) / 3.0), rtol=1e-12)
    assert (got[at["cap"]] == HUGE).all() and (got[at["short-edges"]] == HUGE).all()
    assert ((got[at["under-cap"]] < HUGE) & (got[at["under-cap"]] > 0.95 * HUGE)).all()
    # h2-zero / h1-zero (log1p(-1), log1p(inf)): by value, NaN or not as the oracle decides: close() above
    # the two sides of the r switch differ by the formula, not by much: l / h1 against the logarithm
    for n in ("r-under+", "r-under-", "r-over+", "r-over-"):
        np.testing.assert_allclose(got[at[n]], got[at["h-equal"]], rtol=1e-4)
        assert (got[at[n]] != got[at["h-equal"]]).any()


def test_aniso_branches():
    xyz, tetv, met, at = _mesh_of(_ani_cases(), 6)
    ne = tetv.shape[0]
    gaps = {n: H.ani_gaps(xyz, met, tetv[k]) for n, k in at.items()}
    # (face 3 = edges 12, 01, 02: the face the known answers below are for)
    assert gaps["gap-under"][[0, 1, 3]].max() < 0.045 and (gaps["gap-over"][[0, 1]] > 0.055).all()
    assert gaps["gap-over"][3] == 0.0
    assert (gaps["dd-both-clamped"] == 0).all()
    want = oracle_faces(xyz, tetv, met)
    ctx = make_ctx()
    try:
        got = run_faces(ctx, xyz, tetv, all_faces(ne), met).reshape(ne, 4)
    finally:
        ctx.close()
    close(got, want, "aniso faces")
    assert np.isfinite(got).all()
    assert (got[at["len-one-all"]] == 1.0).all()
    np.testing.assert_allclose(got[at["len-below-one"]], np.exp(-28.0 * 3 * (np.sqrt(0.5) - 1) / 3.0), rtol=1e-12)
    np.testing.assert_allclose(got[at["len-above-one"]], np.exp(-28.0 * 3 * (1 / np.sqrt(3.0) - 1) / 3.0), rtol=1e-12)
    assert (got[at["cap"]] == HUGE).all() and (got[at["short-edges"]] == HUGE).all()
    assert ((got[at["under-cap"]] < HUGE) & (got[at["under-cap"]] > 0.95 * HUGE)).all()
    # clamps: face 3 (edges 12, 01, 02 of CORNER).  dd1-clamped: 01 and 02 are Simpson's (0 + 1 + 4 sqrt .5) / 6, 12 is sqrt 2
    s = (1.0 + 4.0 * np.sqrt(0.5)) / 6.0
    np.testing.assert_allclose(got[at["dd1-clamped"], 3], np.exp(-28.0 * (2 * (s - 1) + 1 / S2 - 1) / 3.0), rtol=1e-12)
    # dd2-clamped: the same two lengths; edge 12 has both ends clamped: length 0, term -1
    np.testing.assert_allclose(got[at["dd2-clamped"], 3], min(np.exp(-28.0 * (2 * (s - 1) - 1) / 3.0), HUGE), rtol=1e-12)
    assert got[at["dd-both-clamped"], 3] == HUGE  # three zero lengths: res = -3
    # the 0.05 switch: midpoint sqrt((1 + g) / 2 + .5) against Simpson on edges 01 and 02
    for n, g, simpson in (("gap-under", 0.04, False), ("gap-over", 0.06, True)):
        mid = np.sqrt(0.5 * (2.0 + g))
        ln = (1.0 + np.sqrt(1.0 + g) + 4.0 * mid) / 6.0 if simpson else mid
        l12 = np.sqrt(2.0 * (1.0 + g))  # both ends (1 + g) I
        res = 2 * (1 / ln - 1) + (1 / l12 - 1)
        np.testing.assert_allclose(got[at[n], 3], np.exp(-28.0 * res / 3.0), rtol=1e-12)


# ---------------------------------------------------------------- k_wgt_mesh: what is written, the mask

@functools.lru_cache(maxsize=None)
def lattice_case():
    m = synth.lattice(synth.CUBE, 4, jitter=0.15, seed=6)  # 384 tetra
    iso = H.graded_sizes(m.xyz) * 1.25  # (sizes for a spacing of 0.2; this lattice's is 0.25)
    ani = synth.solution(synth.F_ANI, m.xyz)
    return m, iso, ani


@pytest.mark.parametrize("tag", [MG_PARBDY, MG_PARBDY | 1, 0x8000], ids=["one-bit", "two-bits", "bit-15"])
@pytest.mark.parametrize("kind", ["iso", "ani", "nomet"])
def test_mesh_weights_mask_and_untouched_entries(kind, tag):
    m, iso, ani = lattice_case()
    met = dict(iso=iso, ani=ani, nomet=None)[kind]
    ne = m.ne
    rng = np.random.default_rng(tag)
    bits = [b for b in (1, MG_PARBDY, 0x8000) if tag & b]
    # per face: nothing, a bit of the tag alone, with others, all of it with others, or only foreign bits
    choice = np.array([0, bits[0], bits[-1] | 0x0412, tag | 0x0030, 0x0412, 0x7FBE & ~tag], np.uint16)
    ftag = choice[rng.integers(0, choice.size, (ne, 4))]
    ftag[10:20] = 0x0412  # used tetra without a tagged face
    xt = (rng.random(ne) < 0.6).astype(np.int32) * rng.integers(1, 1000, ne).astype(np.int32)
    xt[10:20] = 1
    tetv = m.tetv.copy()
    tetv[30:40, 0] = 0  # unused, with an xtetra and tagged faces
    tetv[40:45, 0] *= -1
    xt[30:45] = 1
    ftag[30:45] = tag
    qual0 = np.linspace(0.5, 1.5, ne)
    qual0[::7] = SENT
    want = O.compute_wgt_mesh(m.xyz, tetv, xt, ftag, met, tag, qual0)
    # the mask restated: a face counts when it shares a bit with tag
    W = oracle_faces(m.xyz, m.tetv, met)
    tagged = (ftag.astype(np.int64) & tag) != 0
    touched = (tetv[:, 0] > 0) & (xt != 0)
    restated = np.zeros(ne)
    for f in range(4):
        restated = restated + np.where(tagged[:, f], W[:, f], 0.0)
    ctx = make_ctx()
    try:
        got = run_mesh(ctx, m.xyz, tetv, xt, ftag, met, tag, qual0)
    finally:
        ctx.close()
    assert np.array_equal(got[~touched].view(np.uint64), qual0[~touched].view(np.uint64)), "an entry without xtetra was written"
    close(got[touched], want[touched], "oracle")
    close(got[touched], restated[touched], "mask restated")
    assert (got[10:20] == 0.0).all() and not np.signbit(got[10:20]).any()
    assert touched.sum() > 150 and (~touched).sum() > 100 and (tagged.sum(1)[touched] == 0).sum() >= 10


# ---------------------------------------------------------------- k_wgt_faces: the list

@pytest.mark.parametrize("kind", ["iso", "ani"])
def test_face_list_order_repeats_and_sizes(kind):
    m, iso, ani = lattice_case()
    met = iso if kind == "iso" else ani
    W = oracle_faces(m.xyz, m.tetv, met)
    rng = np.random.default_rng(8)
    ctx = make_ctx()
    try:
        for nface in (0, 1, 255, 256, 257):
            face = np.stack([rng.integers(1, m.ne + 1, nface), rng.integers(0, 4, nface)], 1).astype(np.int32)
            if nface >= 255:
                face[5:9] = [(77, 0), (77, 1), (77, 2), (77, 3)]  # every face of one tetra
                face[100:103] = face[50]  # repeats
                face[nface - 1] = (m.ne, 3)  # the last tetra
            got = run_faces(ctx, m.xyz, m.tetv, face, met)
            assert got.shape == (nface,)
            close(got, W[face[:, 0] - 1, face[:, 1]], f"nface={nface}")
            if nface >= 255:
                assert got[100] == got[50] == got[101]
    finally:
        ctx.close()


# ---------------------------------------------------------------- second trip

@pytest.mark.parametrize("kind", ["iso", "ani"])
def test_second_trip_of_both_weight_kernels(kind):
    """ne = nface = 4 194 304 + 257: past the 16384 blocks of 256 both launches
    are capped at.  Tagged and untagged tetra, tetra without xtetra and unused
    ones lie past the first trip."""
    xyz, tetv, met6, _ = big_mesh()
    nv = xyz.shape[0]
    met = met6 if kind == "ani" else np.ascontiguousarray(0.11 * (0.6 + 0.9 * np.random.default_rng(9).random((nv, 1))))
    ne = tetv.shape[0]
    base = 9 ** 3 * 6
    assert ne == TRIP + 257 and np.array_equal(tetv[base:2 * base], tetv[:base])
    W = oracle_faces(xyz, tetv[:base], met)
    assert ((W < HUGE) & (W > 1)).mean() > 0.3
    k = np.arange(ne)
    xt = (k % 5 != 0).astype(np.int32)
    ftag = np.zeros((ne, 4), np.uint16)
    for f in range(4):
        ftag[:, f] = np.where((k + f) % 3 == 0, MG_PARBDY, 2)
    ftag[k % 11 == 0] = 2  # used, untagged
    tv = tetv.copy()
    tv[k % 13 == 0, 0] = 0
    qual0 = (k % 1000) * 1e-3 + 0.25
    touched = (tv[:, 0] > 0) & (xt != 0)
    tail = slice(TRIP, ne)
    assert touched[tail].sum() > 100 and (~touched[tail]).sum() > 50 and (ftag[tail] == MG_PARBDY).any(1).sum() > 100
    want = O.compute_wgt_mesh(xyz, tv, xt, ftag, met, MG_PARBDY, qual0)
    face = np.stack([(k * 7919) % ne + 1, (k // 3) % 4], 1).astype(np.int32)
    want_f = np.resize(W, (ne, 4))[face[:, 0] - 1, face[:, 1]]
    ctx = make_ctx()
    try:
        got = run_mesh(ctx, xyz, tv, xt, ftag, met, MG_PARBDY, qual0)
        got_f = run_faces(ctx, xyz, tetv, face, met)
    finally:
        ctx.close()
    assert np.array_equal(got[~touched].view(np.uint64), qual0[~touched].view(np.uint64))
    close(got[touched], want[touched], "mesh")
    assert (got[tail][touched[tail]] != qual0[tail][touched[tail]]).all(), "the second trip wrote nothing"
    close(got_f, want_f, "faces")


# ---------------------------------------------------------------- high precision

@pytest.mark.parametrize("ani", [False, True], ids=["iso", "ani"])
def test_device_weights_within_the_oracle_bounds(ani):
    """the inputs and bounds of test_highprec_host.py's weight tests, on the device"""
    xyz, tetv, met = H.wgt_ani_inputs() if ani else H.wgt_iso_inputs()
    val, bnd, _ = H.wgt_reference(ani)
    ctx = make_ctx()
    try:
        got = run_faces(ctx, xyz, tetv, all_faces(tetv.shape[0]), met)
    finally:
        ctx.close()
    rat, tight = H.ratios(got, H.flat(val), H.flat(bnd))
    print(f"device wgt_{'ani' if ani else 'iso'}: n {rat.size} worst error/bound {rat.max():.3g} tight {tight:.3f}")
    assert (rat <= 1.0).all(), np.nonzero(~(rat <= 1.0))[0][:8]


# ---------------------------------------------------------------- the other routes to the same arithmetic

@pytest.mark.parametrize("kind", ["iso", "aniso"])
def test_edge_length_list_within_bounds(kind):
    m, iso, ani = _lattice()
    met = iso if kind == "iso" else ani
    ctx = make_ctx()
    try:
        d = [ctx.upload(a) for a in (m.xyz, m.tetv, met)]
        out, edges, lens = ctx.edge_lengths(d[0], d[1], d[2], want_edges=True)
        edges, lens = edges.download(), lens.download()
    finally:
        ctx.close()
    mine = {(int(min(t[i], t[j])), int(max(t[i], t[j]))) for t in m.tetv for i, j in H.IARE}
    theirs = [(int(min(a, b)), int(max(a, b))) for a, b in edges]
    assert len(theirs) == len(set(theirs)) == len(mine) == out["nedge"] and set(theirs) == mine
    val, bnd = [], []
    for a, b in edges:
        if kind == "iso":
            v, e = H.len_iso(m.xyz[a - 1], m.xyz[b - 1], iso[a - 1, 0], iso[b - 1, 0])
        else:
            v, e, amb = H.len_ani(m.xyz[a - 1], m.xyz[b - 1], ani[a - 1], ani[b - 1])
            assert not amb
        val.append(v)
        bnd.append(e)
    rat, tight = H.ratios(lens, val, bnd)
    print(f"device len_{kind}: n {rat.size} worst error/bound {rat.max():.3g} tight {tight:.3f}")
    assert (rat <= 1.0).all(), np.nonzero(~(rat <= 1.0))[0][:8]
    assert tight > 0.9


@pytest.mark.parametrize("kind", ["iso", "aniso", "aniso-mild"])
def test_graph_weights_within_bounds(kind):
    m, met = lattice_metric(kind)
    ctx = make_ctx()
    try:
        d = [ctx.upload(a) for a in (m.xyz, m.tetv, m.adja, met)]
        xadj, adjncy, adjwgt = [a.download() for a in ctx.metis_graph(d[0], d[1], adja=d[2], met=d[3])]
    finally:
        ctx.close()
    # entries in (tetra, face) order over the faces with a neighbour
    slot, n = {}, 0
    for k in range(m.ne):
        assert xadj[k] == n
        for f in range(4):
            if m.adja[k, f]:
                assert adjncy[n] == m.adja[k, f] // 4 - 1
                slot[(k, f)] = n
                n += 1
    assert xadj[m.ne] == n == adjwgt.size
    skipped, total = graph_weight_check(m, met, lambda k, f: int(adjwgt[slot[(k, f)]]))
    print(kind, "entries", total, "skipped", skipped, "below the cap", int((adjwgt < int(HUGE)).sum()))
    assert total == n and skipped < 0.01 * total
