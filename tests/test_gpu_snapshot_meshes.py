"""Device snapshot (pmmg_hip_build_adjacency, pmmg_hip_build_boundary and the
snapshot inside pmmg_hip_set_background) on unstructured numberings and at its
size edges, against the dictionary definition of tests/snapshot_ref.py.

tests/test_gpu_snapshot.py checks the snapshot on lattices in their generated
numbering; what that leaves out is in the fixtures here (their conditions are
computed in tests/test_snapshot_ref_host.py): the two smallest ids of a tetra
at every pair of positions, chunks of k_face_match on both sides of kMatchCap
and exactly at it, runs of one lane per bucket in a wave, 256-blocks without a
boundary tetra, tria edges of 3 to 6 trias, ne around 64 / 256 / 512, np around
the 24-vertex chunk, and the entry modes of set_background.  Every comparison
is exact; every mesh is below 10k tetra.
"""
import ctypes

import numpy as np
import pytest

import snapshot_ref as R
from parity import GUARD_BYTE, device_view, same_outputs
from parmmg_amd import synth
from parmmg_amd.transfer import TransferContext, _p

KEYS = ("adja", "tet8", "triv", "adjt")
FILL = -77  # what output rows hold before a call


@pytest.fixture(scope="module")
def ctx():
    """one context for the per-fixture and per-size cases: its scratch (SnapCache) is reused across all of them"""
    with TransferContext(0) as c:
        yield c


def _free(*arrays):
    for a in arrays:
        if a is not None:
            a.free()


def _snapshot(ctx, npv, tetv, tref=None, use_tet8=True):
    """the four arrays of one mesh, downloaded"""
    d_tetv = ctx.upload(tetv)
    d_tref = None if tref is None else ctx.upload(tref)
    adja = tet8 = triv = adjt = None
    try:
        adja, tet8 = ctx.build_adjacency(npv, d_tetv)
        if use_tet8:
            triv, adjt = ctx.build_boundary(npv, tet8=tet8, tref=d_tref)
        else:
            triv, adjt = ctx.build_boundary(npv, tetv=d_tetv, adja=adja, tref=d_tref)
        return dict(adja=adja.download(), tet8=tet8.download(), triv=triv.download(), adjt=adjt.download())
    finally:
        _free(d_tetv, d_tref, adja, tet8, triv, adjt)


def _assert_is(out, e):
    for key in KEYS:
        np.testing.assert_array_equal(out[key], getattr(e, key), err_msg=f"{e.name}: {key}")


def _build_boundary(ctx, npv, ne, cap, triv, adjt, tet8=None, tetv=None, adja=None, tref=None):
    """pmmg_hip_build_boundary itself: (return value, *nt)"""
    nt = ctypes.c_int(-1)
    ok = ctx.lib.pmmg_hip_build_boundary(ctx.h, int(npv), int(ne), _p(tet8), _p(tetv), _p(adja), _p(tref), int(cap),
                                         ctypes.byref(nt), _p(triv), _p(adjt))
    return ok, nt.value


# ---------------------------------------------------------------- every fixture, both input forms

@pytest.mark.gpu
@pytest.mark.parametrize("use_tet8", [True, False], ids=["tet8", "tetv+adja"])
@pytest.mark.parametrize("name", list(R.FIXTURES))
def test_fixture_matches_the_definition(ctx, name, use_tet8):
    e = R.fixture(name)
    _assert_is(_snapshot(ctx, e.np, e.tetv, e.tref, use_tet8), e)


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["refs-cube6-d0", "refs-cube8-d25"])
def test_references_change_only_the_boundary(ctx, name):
    """without tref the same mesh gives the plain boundary (tref = NULL is accepted)"""
    e = R.fixture(name)
    plain = R.expected(e.np, e.tetv, name=name + " without references")
    assert plain.nt < e.nt
    _assert_is(_snapshot(ctx, e.np, e.tetv), plain)


# ---------------------------------------------------------------- sizes

PREFIX_NE = (1, 2, 63, 64, 65, 255, 256, 257, 511, 512, 513)


def _prefix(ne, pad):
    base = R.FIXTURES["scr-cube6-d0"]()
    top = R.prefix(base, ne)[0]  # the largest id
    nxt = (top // R.MATCH_VERTS + 1) * R.MATCH_VERTS
    npv = {"top": top, "x24": nxt, "x24+1": nxt + 1, "+3000": top + 3000 + ne % 7}[pad]
    return R.expected(*R.prefix(base, ne, npv), name=f"prefix {ne} np={npv}")


@pytest.mark.gpu
@pytest.mark.parametrize("pad", ["top", "x24", "x24+1"])
@pytest.mark.parametrize("ne", PREFIX_NE)
def test_prefix_sizes(ctx, ne, pad):
    """ne around the wave, the block and two blocks; np equal to the largest
    id, to the next multiple of the 24-vertex chunk and one past it (a last
    chunk of one vertex, whose bucket is empty)"""
    e = _prefix(ne, pad)
    assert e.ne == ne and int(e.tetv.max()) <= e.np
    _assert_is(_snapshot(ctx, e.np, e.tetv, use_tet8=ne % 2 == 1), e)


@pytest.mark.gpu
@pytest.mark.parametrize("ne", [65, 257])
def test_np_far_above_the_largest_id(ctx, ne):
    """some 3000 unused vertices behind the mesh: over a hundred empty chunks, and empty buckets at the end of
    the last chunk that holds a face"""
    e = _prefix(ne, "+3000")
    assert e.np >= int(e.tetv.max()) + 3000 and int(e.tetv.max()) % R.MATCH_VERTS != 0
    _assert_is(_snapshot(ctx, e.np, e.tetv), e)
    _assert_is(_snapshot(ctx, e.np, e.tetv, use_tet8=False), e)


# ---------------------------------------------------------------- the cap contract

@pytest.mark.gpu
@pytest.mark.parametrize("name", ["scr-cube6-d25", "refs-cube6-d0", "one-tetra"])
def test_cap_contract(ctx, name):
    e = R.fixture(name)
    nt = e.nt
    d_tet8, d_tref = ctx.upload(e.tet8), (None if e.tref is None else ctx.upload(e.tref))
    rows = np.full((nt + 7, 3), FILL, np.int32)
    triv, adjt = ctx.upload(rows), ctx.upload(rows)
    try:
        def call(cap, t=triv, a=adjt, tref=d_tref):
            return _build_boundary(ctx, e.np, e.ne, cap, t, a, tet8=d_tet8, tref=tref)

        def refill():
            for a in (triv, adjt):
                assert ctx.lib.pmmg_hip_memcpy_h2d(ctx.h, _p(a), _p(rows), rows.nbytes)

        # too small a capacity: 0, *nt set, nothing written
        for cap in (nt - 1, 0):
            assert call(cap) == (0, nt), cap
            assert "exceed the capacity" in ctx.error()
            np.testing.assert_array_equal(triv.download(), rows)
            np.testing.assert_array_equal(adjt.download(), rows)
        assert call(0, None, None) == (0, nt)  # the counting call
        # cap = nt + 7: nt rows, the seven behind them keep their fill
        assert call(nt + 7) == (1, nt)
        for got, want in ((triv.download(), e.triv), (adjt.download(), e.adjt)):
            np.testing.assert_array_equal(got[:nt], want)
            np.testing.assert_array_equal(got[nt:], rows[nt:])
        # cap = nt: exactly nt rows; adjt = NULL is accepted and leaves adjt alone
        refill()
        assert call(nt, a=None) == (1, nt)
        np.testing.assert_array_equal(triv.download()[:nt], e.triv)
        np.testing.assert_array_equal(triv.download()[nt:], rows[nt:])
        np.testing.assert_array_equal(adjt.download(), rows)
        assert call(nt) == (1, nt)
        np.testing.assert_array_equal(adjt.download()[:nt], e.adjt)
        # tref = NULL is accepted: the plain boundary
        plain = R.expected(e.np, e.tetv)
        refill()
        assert call(nt + 7, tref=None) == (1, plain.nt)
        np.testing.assert_array_equal(triv.download()[:plain.nt], plain.triv)
        np.testing.assert_array_equal(adjt.download()[:plain.nt], plain.adjt)
        np.testing.assert_array_equal(triv.download()[plain.nt:], rows[plain.nt:])
    finally:
        _free(d_tet8, d_tref, triv, adjt)


# ---------------------------------------------------------------- guard zones

@pytest.mark.gpu
@pytest.mark.parametrize("use_tet8", [True, False], ids=["tet8", "tetv+adja"])
@pytest.mark.parametrize("name", ["refs-cube8-d25", "star257", "interior-cube8", "one-tetra"])
def test_nothing_is_written_outside_the_arrays(name, use_tet8):
    """Every output, and tetv / tref as inputs, 16 bytes past a 256-byte
    boundary (the header allows no smaller alignment) between guard zones: the
    zones stay untouched, the inputs unchanged, the outputs right to their
    last row."""
    e = R.fixture(name)
    with TransferContext(0) as c:
        allocs = {}

        def dv(key, arr):
            view, allocs[key] = device_view(c, arr, 16)
            return view

        try:
            tetv = dv("tetv", e.tetv)
            tref = None if e.tref is None else dv("tref", e.tref)
            adja, tet8 = dv("adja", np.full((e.ne, 4), FILL, np.int32)), dv("tet8", np.full((e.ne, 8), FILL, np.int32))
            triv, adjt = dv("triv", np.full((e.nt, 3), FILL, np.int32)), dv("adjt", np.full((e.nt, 3), FILL, np.int32))
            c.build_adjacency(e.np, tetv, out=(adja, tet8))
            form = dict(tet8=tet8) if use_tet8 else dict(tetv=tetv, adja=adja)
            assert _build_boundary(c, e.np, e.ne, 0, None, None, tref=tref, **form) == (0, e.nt)
            assert _build_boundary(c, e.np, e.ne, e.nt, triv, adjt, tref=tref, **form) == (1, e.nt)
            _assert_is(dict(adja=adja.download(), tet8=tet8.download(), triv=triv.download(), adjt=adjt.download()), e)
            np.testing.assert_array_equal(tetv.download(), e.tetv)
            if tref is not None:
                np.testing.assert_array_equal(tref.download(), e.tref)
            for key, al in allocs.items():
                al.check(f"{name}: {key}")
                before, after = al.zones()
                assert before.size == 256 + 16 and after.size == 256 and GUARD_BYTE == 0xA5
        finally:
            for al in allocs.values():
                al.free()


# ---------------------------------------------------------------- determinism, history

@pytest.mark.gpu
def test_runs_give_identical_bytes():
    """The slot a face gets in its bucket depends on the order of the atomics;
    the result must not.  Three runs on one context and one on a fresh one."""
    e = R.fixture("scr-cube8-d25")
    with TransferContext(0) as c:
        runs = [_snapshot(c, e.np, e.tetv, use_tet8=j != 1) for j in range(3)]
    with TransferContext(0) as c:
        runs.append(_snapshot(c, e.np, e.tetv))
    _assert_is(runs[0], e)
    for r in runs[1:]:
        for key in KEYS:
            assert r[key].tobytes() == runs[0][key].tobytes(), key


def _duplicated(tetv, k=0):
    """the mesh with tetra k a second time (its vertices reordered): four faces of three tetra"""
    return np.ascontiguousarray(np.concatenate([tetv, tetv[k:k + 1, [1, 0, 2, 3]]]), dtype=np.int32)


def _graph(c, npv, tetv):
    """the unweighted element graph from tetv alone: the adjacency is built first, in the context's SnapCache"""
    xyz, d_tetv = c.upload(np.zeros((npv, 3))), c.upload(tetv)
    xadj, adjncy, _ = c.metis_graph(xyz, d_tetv, weights=False)
    out = xadj.download(), adjncy.download()
    _free(xyz, d_tetv, xadj, adjncy)
    return out


@pytest.mark.gpu
def test_history_on_one_context():
    """Meshes of very different sizes, a call that shares the scratch, its
    release and a rejected build, in a row on one context: every result is
    what a fresh context gives (the definition's arrays)."""
    big, refs, small = R.fixture("scr-cube10-d0"), R.fixture("refs-cube6-d0"), R.fixture("scr-cube6-d0")
    star, one = R.fixture("star257"), R.fixture("one-tetra")
    with TransferContext(0) as fresh:
        graph_fresh = _graph(fresh, refs.np, refs.tetv)
    # xadj by the definition: one arc per face with a neighbour
    np.testing.assert_array_equal(graph_fresh[0], np.concatenate([[0], np.cumsum((refs.adja > 0).sum(axis=1))]))
    with TransferContext(0) as c:
        _assert_is(_snapshot(c, big.np, big.tetv), big)                          # 1
        _assert_is(_snapshot(c, one.np, one.tetv), one)                          # 2
        _assert_is(_snapshot(c, star.np, star.tetv, use_tet8=False), star)       # 3
        _assert_is(_snapshot(c, refs.np, refs.tetv, refs.tref), refs)            # 4
        for a, b in zip(_graph(c, refs.np, refs.tetv), graph_fresh):             # 5
            np.testing.assert_array_equal(a, b)
        _assert_is(_snapshot(c, one.np, one.tetv, use_tet8=False), one)
        c.release_scratch()                                                      # 6
        _assert_is(_snapshot(c, star.np, star.tetv), star)
        bad = c.upload(_duplicated(R.strip_star(300)[1]))                        # 7
        with pytest.raises(RuntimeError, match="more than two"):
            c.build_adjacency(326, bad)
        _assert_is(_snapshot(c, small.np, small.tetv), small)                    # 8
        _assert_is(_snapshot(c, big.np, big.tetv, use_tet8=False), big)


# ---------------------------------------------------------------- rejections

@pytest.mark.gpu
@pytest.mark.parametrize("T", [300, 100], ids=["in-place", "lds"])
def test_duplicated_tetra_is_rejected_on_both_match_paths(ctx, T):
    """Three tetra on a face, in the hub's bucket: 3 T + 3 entries in the first
    chunk, above kMatchCap for T = 300 (matched in place: `found > 1`) and below
    it for T = 100 (the LDS hash finds the mate taken).  An error return of
    in-range code; a valid build right after succeeds."""
    npv, tetv = R.strip_star(T)
    bad = _duplicated(tetv, T // 2)
    assert (R.chunk_sizes(npv, bad)[0] > R.MATCH_CAP) == (T == 300) and R.adjacency(bad)[1]
    d = ctx.upload(bad)
    try:
        with pytest.raises(RuntimeError, match="more than two"):
            ctx.build_adjacency(npv, d)
    finally:
        _free(d)
    _assert_is(_snapshot(ctx, npv, tetv), R.expected(npv, tetv, name=f"strip_star({T})"))


@pytest.mark.gpu
@pytest.mark.parametrize("bad_id", ["0", "np+1"])
def test_id_out_of_range_in_a_partial_wave_is_rejected(ctx, bad_id):
    e = R.fixture("scr-cube6-d25")
    assert e.ne % 64 not in (0, 1)  # the last wave is partial
    bad = e.tetv.copy()
    k = e.ne - 2  # inside it
    assert k // 64 == (e.ne - 1) // 64
    bad[k, 2] = 0 if bad_id == "0" else e.np + 1
    d = ctx.upload(bad)
    try:
        with pytest.raises(RuntimeError, match="vertex ids"):
            ctx.build_adjacency(e.np, d)
    finally:
        _free(d)
    _assert_is(_snapshot(ctx, e.np, e.tetv), e)


# ---------------------------------------------------------------- the entry modes of set_background

class _Case:
    """A scrambled background (coordinates carried along, orientation kept)
    with its arrays by the definition, solutions and new points."""

    def __init__(self):
        lat = synth.lattice(synth.CUBE, 5)
        self.np, self.tetv, self.xyz, _ = R.scrambled_mesh(lat, 9, even=True)
        e = R.expected(self.np, self.tetv, name="scrambled cube 5")
        self.adja, self.triv, self.adjt = e.adja, e.triv, e.adjt
        perm = np.random.default_rng(2).permutation(e.nt)
        self.triv_perm = np.ascontiguousarray(e.triv[perm])
        self.adjt_perm = R.tria_adjacency(self.triv_perm)
        self.met = synth.solution(synth.F_ANI, self.xyz)
        self.fields = [synth.solution(w, self.xyz) for w in (synth.F_SCALAR, synth.F_VECTOR, synth.F_TENSOR)]
        new = synth.lattice(synth.CUBE, 6, jitter=0.2, with_tetra=False)
        self.q, self.pclass = new.xyz, synth.classes(new)
        self.hausd = 0.01


@pytest.fixture(scope="module")
def case():
    return _Case()


def _locate(c, cs, host_mode, solutions=True):
    """set_solutions (unless they are set) + locate_interp on the background that is set: the outputs, downloaded"""
    n = cs.q.shape[0]
    up = (lambda a: a) if host_mode else c.upload
    if solutions:
        c.set_solutions(up(cs.met), [up(f) for f in cs.fields])
    mo = up(np.full((n, cs.met.shape[1]), np.nan))
    fo = [up(np.full((n, f.shape[1]), np.nan)) for f in cs.fields]
    el, hit = up(np.zeros(n, np.int32)), up(np.zeros(n, np.int8))
    c.locate_interp(up(cs.q), up(cs.pclass), mo, fo, el, hit)
    dl = (lambda a: a) if host_mode else (lambda a: a.download())
    return dict(met=dl(mo), fields=[dl(f) for f in fo], elem=dl(el), hit=dl(hit))


def _transfer(cs, host_mode, adja, triv, adjt):
    with TransferContext(0) as c:
        up = (lambda a: a) if host_mode else (lambda a: None if a is None else c.upload(a))
        c.set_background(up(cs.xyz), up(cs.tetv), up(adja), up(triv), up(adjt), cs.hausd)
        return _locate(c, cs, host_mode)


@pytest.mark.gpu
@pytest.mark.parametrize("host_mode", [True, False], ids=["host", "device"])
def test_set_background_modes_give_identical_transfers(case, host_mode):
    """The four modes of pmmg_hip_set_background — everything given; tetv
    only; tetv + adja with the trias built; triv given, adjt built — give
    bit-identical elem, hit, metric and fields.  The all-given run has the
    dictionary's arrays.  The mode "triv given, adjt built" gets the trias in
    a permuted order, and is compared with the all-given run on the same
    permuted triv and the dictionary's adjt of it (elem of a surface point is
    a tria index)."""
    cs = case
    ref = _transfer(cs, host_mode, cs.adja, cs.triv, cs.adjt)
    moved = cs.pclass != 0
    assert ((ref["hit"][moved] & 15) != 0).all() and ((cs.pclass == 2).sum() > 0) and ((cs.pclass == 1).sum() > 0)
    same_outputs(_transfer(cs, host_mode, None, None, None), ref)          # tetv only
    same_outputs(_transfer(cs, host_mode, cs.adja, None, None), ref)       # tetv + adja, trias built
    same_outputs(_transfer(cs, host_mode, cs.adja, cs.triv, None), ref)    # triv given, adjt built
    ref_perm = _transfer(cs, host_mode, cs.adja, cs.triv_perm, cs.adjt_perm)
    same_outputs(_transfer(cs, host_mode, cs.adja, cs.triv_perm, None), ref_perm)
    same_outputs(_transfer(cs, host_mode, None, cs.triv_perm, None), ref_perm)  # (and with the adjacency built too)
    # (the permuted order shows in elem: a surface point's element is a tria index)
    assert not np.array_equal(ref_perm["elem"], ref["elem"])


@pytest.mark.gpu
@pytest.mark.parametrize("host_mode", [True, False], ids=["host", "device"])
def test_failed_tria_adjacency_drops_the_background(case, host_mode):
    """triv given, adjt built, with a tria vertex id of np + 1: device mode
    fails at set_background ("tria vertex ids"); host mode defers the snapshot
    and the next call reports it.  Every later locate_interp fails cleanly
    until a valid set_background — what test_failed_snapshot_drops_the_background
    asserts for the adjacency."""
    cs = case
    bad = cs.triv_perm.copy()
    bad[bad.shape[0] // 2, 1] = cs.np + 1
    ref = _transfer(cs, host_mode, cs.adja, cs.triv_perm, cs.adjt_perm)
    with TransferContext(0) as c:
        if host_mode:
            c.set_background(cs.xyz, cs.tetv, cs.adja, bad, None, cs.hausd)  # snapshot deferred
            c.set_solutions(cs.met, cs.fields)  # uploads beside the snapshot (does not join it)
            with pytest.raises(RuntimeError, match="tria vertex ids"):
                _locate(c, cs, True, solutions=False)
        else:
            with pytest.raises(RuntimeError, match="tria vertex ids"):
                c.set_background(c.upload(cs.xyz), c.upload(cs.tetv), c.upload(cs.adja), c.upload(bad), None, cs.hausd)
        for _ in range(2):
            with pytest.raises(RuntimeError, match="locate_interp failed"):
                _locate(c, cs, host_mode, solutions=False)
        # a valid background makes the context usable again
        up = (lambda a: a) if host_mode else c.upload
        c.set_background(up(cs.xyz), up(cs.tetv), up(cs.adja), up(cs.triv_perm), None, cs.hausd)
        same_outputs(_locate(c, cs, host_mode), ref)
