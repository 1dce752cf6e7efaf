"""pmmg_hip_tetra_qual (k_tetra_qual, pmmg_quality.hip) on every branch of
MMG5_caltet_iso / _ani, at the sizes where the launch and the minimum's
reduction change shape, across calls of one context, under bad arguments, and
against the 50-digit reference of tests/highprec.py.

Contract: qual is bit-identical to the oracle's (compared as uint64), except
that both are NaN where either is (payload and sign of a NaN differ between x86
and the device); minqual is equal.  Every array sits behind parity.device_view
at its smallest legal offset (tetv + 16, xyz / met / qual + 8); after every call
the guard zones of all of them are checked and the inputs are downloaded and
compared with what was uploaded."""
import ctypes
import functools

import numpy as np
import pytest

import highprec as H
from oracle import oracle as O
from parity import device_view, make_ctx
from parmmg_amd import synth

pytestmark = pytest.mark.gpu

SENT = np.array([0x7FF8C0DE0000F00D], np.uint64).view(np.float64)[0]  # a NaN with a payload of its own
I6 = np.array([1.0, 0.0, 0.0, 1.0, 0.0, 1.0])
TRIP = 16384 * 256  # elements of one grid-stride trip: 4 194 304


def same_qual(got, want, what=""):
    gn, wn = np.isnan(got), np.isnan(want)
    assert np.array_equal(gn, wn), (what, np.nonzero(gn != wn)[0][:8])
    g, w = got.view(np.uint64)[~gn], want.view(np.uint64)[~wn]
    assert np.array_equal(g, w), (what, int((g != w).sum()), np.nonzero(~gn)[0][np.nonzero(g != w)[0][:8]])


def run_qual(ctx, xyz, tetv, met=None, met_size=None, null_met=False):
    """One pmmg_hip_tetra_qual over guarded views; returns (qual, minqual).
    met_size defaults to the metric's width (0 without one); null_met passes
    met = NULL whatever the metric."""
    tetv = np.ascontiguousarray(tetv, np.int32).reshape(-1, 4)
    ne = tetv.shape[0]
    ins = dict(xyz=(np.ascontiguousarray(xyz, np.float64), 8), tetv=(tetv, 16))
    if met is not None and not null_met:
        ins["met"] = (np.ascontiguousarray(met, np.float64), 8)
    views, allocs = {}, {}
    try:
        for name, (a, off) in ins.items():
            views[name], allocs[name] = device_view(ctx, a, off)
        views["qual"], allocs["qual"] = device_view(ctx, np.full(ne, SENT), 8)
        ms = (0 if met is None else met.shape[1]) if met_size is None else met_size
        mn = ctypes.c_double(-1.0)
        ok = ctx.lib.pmmg_hip_tetra_qual(ctx.h, xyz.shape[0], ctypes.c_void_p(views["xyz"].ptr), ne,
                                         ctypes.c_void_p(views["tetv"].ptr), ms,
                                         ctypes.c_void_p(views["met"].ptr) if "met" in views else None,
                                         ctypes.c_void_p(views["qual"].ptr), ctypes.byref(mn))
        assert ok, ctx.error()
        qual = views["qual"].download()
        for name, al in allocs.items():
            al.check(name)
        for name, (a, _) in ins.items():
            assert np.array_equal(views[name].download().view(np.uint8), a.view(np.uint8)), f"{name} was written"
        return qual, mn.value
    finally:
        for al in allocs.values():
            al.free()


def check_against_oracle(ctx, xyz, tetv, met=None, what=""):
    qual, mn = run_qual(ctx, xyz, tetv, met)
    want, mn_ref = O.tetra_qual(xyz, np.ascontiguousarray(tetv, np.int32).reshape(-1, 4),
                                met if met is not None and met.shape[1] == 6 else None)
    same_qual(qual, want, what)
    assert mn == mn_ref, (what, mn, mn_ref)
    return qual, mn


# ---------------------------------------------------------------- branches

def _corner(a):
    """the corner tetra of edge a: vol = a^3 exactly up to rounding, rap = 9 a^2"""
    return np.array([[0, 0, 0], [a, 0, 0], [0, a, 0], [0, 0, a]], np.float64)


def _diag(a, b, c):
    return np.array([a, 0.0, 0.0, b, 0.0, c])


FLAT = np.array([[0, 0, 0], [2, 0, 0], [0, 2, 0], [2, 2, 0]], np.float64)  # exactly coplanar
NANROW = "nanrow"
# kind -> (vertices, vertex tensors (one for all four, or NANROW), unused v[0] or None, iso result, aniso result)
KINDS = {
    "vol-under-EPSD2": (_corner((0.9e-200) ** (1 / 3)), I6, None, "zero", "pos"),  # iso: vol < EPSD2; ani: vol > 0
    "vol-over-EPSD2": (_corner((1.1e-200) ** (1 / 3)), I6, None, "pos", "pos"),
    "coplanar": (FLAT, I6, None, "zero", "zero"),  # vol == 0: iso vol < EPSD2, ani vol <= 0
    "inverted": (H.REG[[0, 2, 1, 3]], I6, None, "zero", "zero"),
    "det-under-EPSOK": (H.REG, _diag(*[(0.9e-20) ** (1 / 3)] * 3), None, "pos", "zero"),
    "det-over-EPSOK": (H.REG, _diag(*[(1.1e-20) ** (1 / 3)] * 3), None, "pos", "pos"),
    "det-negative": (H.REG, _diag(1.0, 1.0, -1.0), None, "pos", "zero"),
    "indefinite-rap-negative": (H.REG, _diag(-1.0, -1.0, 1.0), None, "pos", "nan"),  # det = 1, rap = -16
    "nan-row": (H.REG, NANROW, None, "pos", "nan"),  # a failed MMG5_invmat over a NaN-filled buffer
    "overflow-1e120": (H.REG * 1e120, I6, None, "nan", "nan"),  # vol and rap^1.5 overflow: inf / inf
    "unused-zero": (H.REG, I6, 0, "zero", "zero"),
    "unused-negative": (H.REG, I6, -7, "zero", "zero"),
}
COPIES = 3  # each kind at k, k + 128, k + 256: three different waves, two blocks


@functools.lru_cache(maxsize=None)
def branch_mesh():
    """(xyz, tetv, met, where): 384 regular tetra in the identity metric with
    the KINDS planted at where[kind] = their indices"""
    ne = 128 * COPIES
    xyz = np.tile(H.REG, (ne, 1))
    met = np.tile(I6, (4 * ne, 1))
    tetv = np.arange(1, 4 * ne + 1, dtype=np.int32).reshape(-1, 4)
    where = {}
    for j, (kind, (p, m, unused, _, _)) in enumerate(KINDS.items()):
        where[kind] = [c * 128 + 3 + 10 * j for c in range(COPIES)]
        for k in where[kind]:
            xyz[4 * k:4 * k + 4] = p
            if isinstance(m, str):
                met[4 * k + 2] = np.nan
            else:
                met[4 * k:4 * k + 4] = m
            if unused is not None:
                tetv[k, 0] = unused
    assert len({k // 64 for k in where["nan-row"]}) == COPIES
    return xyz, tetv, met, where


@pytest.mark.parametrize("ani", [False, True], ids=["iso", "ani"])
def test_every_branch(ani):
    xyz, tetv, met, where = branch_mesh()
    ctx = make_ctx()
    try:
        qual, mn = check_against_oracle(ctx, xyz, tetv, met if ani else None, "branches")
    finally:
        ctx.close()
    assert mn == 0.0
    special = {k for ks in where.values() for k in ks}
    plain = np.array([k for k in range(tetv.shape[0]) if k not in special])
    assert (qual[plain] == qual[plain[0]]).all() and abs(qual[plain[0]] * 12 * np.sqrt(3) - 1) < 1e-14
    for kind, ks in where.items():
        expect = KINDS[kind][4 if ani else 3]
        for k in ks:
            q = qual[k]
            if expect == "zero":
                assert q == 0.0 and not np.signbit(q), (kind, k, q)
            elif expect == "nan":
                assert np.isnan(q), (kind, k, q)
            else:
                assert 0.0 < q < np.inf, (kind, k, q)
    # the threshold pair scores like any corner tetra once it is past the test: 1 / 27 (iso and M = I)
    over = qual[where["vol-over-EPSD2"][0]]
    assert abs(over * 27 - 1) < 1e-14
    if ani:
        assert abs(qual[where["vol-under-EPSD2"][0]] * 27 - 1) < 1e-14


def test_iso_ignores_the_metric():
    """met_size = 1 with a metric, with met = NULL, and met_size = 0: the same bytes"""
    m = synth.lattice(synth.CUBE, 3, jitter=0.2, seed=2)
    sizes = synth.solution(synth.F_ISO, m.xyz)
    assert sizes.shape[1] == 1
    ctx = make_ctx()
    try:
        a, mna = run_qual(ctx, m.xyz, m.tetv, sizes)
        b, mnb = run_qual(ctx, m.xyz, m.tetv, sizes, met_size=1, null_met=True)
        c, mnc = check_against_oracle(ctx, m.xyz, m.tetv, None)
        d, mnd = run_qual(ctx, m.xyz, m.tetv, np.full_like(sizes, np.nan))
    finally:
        ctx.close()
    for x, mn in ((a, mna), (b, mnb), (d, mnd)):
        assert np.array_equal(x.view(np.uint64), c.view(np.uint64)) and mn == mnc
    assert (c > 0).all()


# ---------------------------------------------------------------- sizes

@functools.lru_cache(maxsize=None)
def small_mesh():
    """(xyz, tetv, met6, worst): a jittered 3^3 lattice (162 tetra) and, on four
    vertices of its own, one thin tetra whose quality is below every other's in
    both metric kinds; worst = its tetv row"""
    m = synth.lattice(synth.CUBE, 3, jitter=0.2, seed=2)
    thin = np.array([[0.1, 0.1, 0.1], [0.6, 0.1, 0.1], [0.1, 0.6, 0.1], [0.3, 0.3, 0.1005]])
    xyz = np.ascontiguousarray(np.vstack([m.xyz, thin]))
    met = synth.solution(synth.F_ANI, xyz)
    worst = np.arange(m.np + 1, m.np + 5, dtype=np.int32)
    for me in (None, met):
        q, _ = O.tetra_qual(xyz, np.vstack([m.tetv, worst]), me)
        assert 0 < q[-1] < 0.05 * q[:-1].min()
    for a in (xyz, met):
        a.setflags(write=False)
    return xyz, np.ascontiguousarray(m.tetv), met, worst


def tiled(tetv, ne):
    return np.ascontiguousarray(np.resize(tetv, (ne, 4)))


def positions(ne):
    """first, last, start of the partial last wave, start of the partial last block"""
    return sorted({p for p in (0, ne - 1, ne - ne % 64, ne - ne % 256) if 0 <= p < ne})


def holes(tetv):
    """a whole wave (64..127) and, where there is one, a whole block (256..511) of unused tetra"""
    ne = tetv.shape[0]
    if ne >= 255:
        tetv[64:128, 0] = 0
    if ne >= 511:
        tetv[256:512, 0] = -tetv[256:512, 0]


SIZES = (0, 1, 63, 64, 65, 255, 256, 257, 511, 513)


@pytest.mark.parametrize("ani", [False, True], ids=["iso", "ani"])
def test_sizes_and_where_the_minimum_sits(ani):
    xyz, base, met6, worst = small_mesh()
    met = met6 if ani else None
    qworst = O.tetra_qual(xyz, worst[None, :], met)[0][0]
    ctx = make_ctx()
    try:
        for ne in SIZES:
            if ne == 0:
                qual, mn = check_against_oracle(ctx, xyz, np.zeros((0, 4), np.int32), met, "ne=0")
                assert qual.size == 0 and mn == 2.0
                continue
            for pos in positions(ne):
                tetv = tiled(base, ne)
                holes(tetv)
                tetv[pos] = worst
                qual, mn = check_against_oracle(ctx, xyz, tetv, met, f"ne={ne} pos={pos}")
                assert qual[pos] == qworst and mn == 20.7846096908265 * qworst, (ne, pos, mn)
                assert (qual[tetv[:, 0] <= 0] == 0.0).all()
            tetv = tiled(base, ne)
            tetv[:, 0] = np.where(np.arange(ne) % 2 == 0, 0, -tetv[:, 0])  # all unused
            qual, mn = check_against_oracle(ctx, xyz, tetv, met, f"ne={ne} unused")
            assert mn == 2.0 and not qual.view(np.uint64).any()
    finally:
        ctx.close()


# ---------------------------------------------------------------- second trip

@functools.lru_cache(maxsize=None)
def big_mesh():
    """(xyz, tetv [TRIP + 257, 4], met6, worst): the tetra of a jittered 9^3
    lattice tiled past the grid's cap of 16384 blocks of 256"""
    m = synth.lattice(synth.CUBE, 9, jitter=0.15, seed=4)
    thin = np.array([[0.1, 0.1, 0.1], [0.6, 0.1, 0.1], [0.1, 0.6, 0.1], [0.3, 0.3, 0.1005]])
    xyz = np.ascontiguousarray(np.vstack([m.xyz, thin]))
    met = synth.solution(synth.F_ANI, xyz)
    worst = np.arange(m.np + 1, m.np + 5, dtype=np.int32)
    tetv = tiled(m.tetv, TRIP + 257)
    for a in (xyz, met, tetv):
        a.setflags(write=False)
    return xyz, tetv, met, worst


@pytest.mark.parametrize("case", ["iso", "ani", "first-trip"])
def test_second_trip_of_the_grid_stride_loop(case):
    xyz, base, met6, worst = big_mesh()
    met = met6 if case == "ani" else None
    tetv = base.copy()
    ne = tetv.shape[0]
    if case == "first-trip":
        pos = 12345
        tetv[TRIP:, 0] = 0
    else:
        pos = ne - 3
    tetv[pos] = worst
    ctx = make_ctx()
    try:
        qual, mn = check_against_oracle(ctx, xyz, tetv, met, case)
    finally:
        ctx.close()
    qworst = O.tetra_qual(xyz, worst[None, :], met)[0][0]
    assert qual[pos] == qworst and mn == 20.7846096908265 * qworst
    if case == "first-trip":
        assert not qual[TRIP:].view(np.uint64).any()
    else:
        assert (qual[TRIP:] > 0).all()


# ---------------------------------------------------------------- history

def test_minimum_does_not_survive_a_call():
    """One context: A (a thin tetra, minimum about 1e-3), B (minimum about
    0.5), no tetra, all unused, A again.  The device's minimum cell is reused:
    each call must start it afresh."""
    xyz, base, _, worst = small_mesh()
    A = tiled(base, 300)
    A[137] = worst
    B = tiled(base, 300)
    unused = B.copy()
    unused[:, 0] = 0
    ctx = make_ctx()
    try:
        qa, mna = check_against_oracle(ctx, xyz, A, None, "A")
        qb, mnb = check_against_oracle(ctx, xyz, B, None, "B")
        _, mn0 = check_against_oracle(ctx, xyz, np.zeros((0, 4), np.int32), None, "ne=0")
        _, mnu = check_against_oracle(ctx, xyz, unused, None, "unused")
        qa2, mna2 = check_against_oracle(ctx, xyz, A, None, "A again")
    finally:
        ctx.close()
    assert mna < 0.02 < 0.2 < mnb < 1.0 and (mn0, mnu) == (2.0, 2.0) and mna2 == mna
    assert np.array_equal(qa.view(np.uint64), qa2.view(np.uint64))


# ---------------------------------------------------------------- arguments

def test_bad_arguments_are_refused_and_write_nothing():
    xyz, base, met6, _ = small_mesh()
    tetv = tiled(base, 100)
    ctx = make_ctx()
    allocs = []
    try:
        def dv(a, off):
            v, al = device_view(ctx, a, off)
            allocs.append(al)
            return v

        x, t, t8, m = dv(xyz, 8), dv(tetv, 16), dv(tetv, 8), dv(met6, 8)
        q = dv(np.full(100, SENT), 8)
        mn = ctypes.c_double(-1.0)
        p = lambda v: None if v is None else ctypes.c_void_p(v.ptr)
        cases = {"met_size=3": (100, t, 3, m, ctypes.byref(mn)), "met_size=6 without met": (100, t, 6, None, ctypes.byref(mn)),
                 "tetv at +8": (100, t8, 6, m, ctypes.byref(mn)), "minqual=NULL": (100, t, 6, m, None),
                 "ne=-1": (-1, t, 6, m, ctypes.byref(mn))}
        for what, (ne, tv, ms, mv, pmn) in cases.items():
            ok = ctx.lib.pmmg_hip_tetra_qual(ctx.h, xyz.shape[0], p(x), ne, p(tv), ms, p(mv), p(q), pmn)
            assert ok == 0 and "tetra_qual" in ctx.error(), (what, ok, ctx.error())
            assert (q.download().view(np.uint64) == np.array([SENT]).view(np.uint64)[0]).all(), what
            assert mn.value == -1.0, what
        for al in allocs:
            al.check("arguments")
        # the context still works
        qual, _ = check_against_oracle(ctx, xyz, tetv, met6, "after the refusals")
        assert (qual > 0).all()
    finally:
        for al in allocs:
            al.free()
        ctx.close()


# ---------------------------------------------------------------- high precision

@pytest.mark.parametrize("ani", [False, True], ids=["iso", "ani"])
def test_device_quality_within_the_oracle_bounds(ani):
    """the inputs and bounds of test_highprec_host.py::test_oracle_quality_within_bounds, on the device"""
    xyz, tetv, _ = H.qual_geometry()
    met = H.qual_tensors() if ani else None
    val, bnd = H.qual_reference(ani)
    ctx = make_ctx()
    try:
        qual, _ = check_against_oracle(ctx, xyz, tetv, met, "highprec")
    finally:
        ctx.close()
    rat, tight = H.ratios(qual, val, bnd)
    print(f"device qual_{'ani' if ani else 'iso'}: n {rat.size} worst error/bound {rat.max():.3g} tight {tight:.3f}")
    assert (rat <= 1.0).all(), np.nonzero(~(rat <= 1.0))[0][:8]
