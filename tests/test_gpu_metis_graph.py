"""pmmg_hip_metis_graph (PMMG_graph_meshElts2metis on the device) against the
numpy restatement of tests/test_metis_graph.py, exactly (runs on the MI355X).

The comparison of adjwgt is exact because the fixture keeps every uncapped
weight at least 1e-11 relative away from an integer while the device weight
is within 1e-13 of the oracle's (test_metis_graph.py asserts the former,
test_wgt.py the latter).  The weights are tied a second way, without the
oracle: adjwgt equals max(trunc(w), 1) of the same context's
compute_wgt_faces over the interior-face list, bit for bit.

Sizes: 1, 2 (one wave, hardly any entry), 63 / 64 / 65 (a wave's edge), 255 /
256 / 257 (a block's edge), 4097 (17 blocks, the last with one tetra), the
whole fixture (6000 tetra, 24 blocks).  A band of 512 cut tetra gives two
whole blocks without an entry between full ones."""
import ctypes

import numpy as np
import pytest

from parity import make_case, run_gpu, same_outputs
from parmmg_amd import _native, synth
from parmmg_amd.transfer import DeviceArray, TransferContext, pack_tet8
from test_metis_graph import HUGE, KINDS, cut, fixture, graph_ref

GUARD = 256
FILL = 0xA5
SENT = -7


@pytest.fixture(scope="module")
def ctx():
    with TransferContext(0) as c:
        yield c


@pytest.fixture(scope="module")
def dev(ctx):
    """the fixture's arrays on the device (never modified)"""
    bg, mets = fixture()
    return dict(xyz=ctx.upload(bg.xyz), tetv=ctx.upload(bg.tetv), adja=ctx.upload(bg.adja),
                tet8=ctx.upload(pack_tet8(bg.tetv, bg.adja)), iso=ctx.upload(mets["iso"]),
                aniso=ctx.upload(mets["aniso"]), nomet=None, noweights=None)


def graph(ctx, dev, kind, tetv=None, adja="given", tet8=None):
    """metis_graph of the fixture (or of the given device tetra arrays) as numpy arrays"""
    tetv = dev["tetv"] if tetv is None and tet8 is None else tetv
    adja = dev["adja"] if isinstance(adja, str) else adja
    x, a, w = ctx.metis_graph(dev["xyz"], tetv, adja=None if tet8 is not None else adja, tet8=tet8, met=dev[kind],
                              weights=kind != "noweights")
    out = x.download(), a.download(), (None if w is None else w.download())
    for d in (x, a, w):
        if d is not None:
            d.free()
    return out


def assert_graph(got, want):
    np.testing.assert_array_equal(got[0], want[0])
    np.testing.assert_array_equal(got[1], want[1])
    assert (got[2] is None) == (want[2] is None)
    if want[2] is not None:
        np.testing.assert_array_equal(got[2], want[2])


def up(ctx, *arrays):
    return [ctx.upload(np.ascontiguousarray(a)) for a in arrays]


# ---------------------------------------------------------------- 1. values

@pytest.mark.gpu
@pytest.mark.parametrize("kind", KINDS)
def test_values(ctx, dev, kind):
    bg, _ = fixture()
    got = graph(ctx, dev, kind)
    want = graph_ref(bg.tetv, bg.adja, kind)
    assert got[0][-1] == 22800
    assert_graph(got, want)
    if kind == "noweights":
        return
    # the existing face-list kernel on the same faces, truncated as the reference truncates
    k, f = np.nonzero(bg.adja)
    faces = ctx.upload(np.ascontiguousarray(np.stack([k + 1, f], axis=1).astype(np.int32)))
    wf = ctx.compute_wgt_faces(dev["xyz"], dev["tetv"], faces, dev[kind])
    w = wf.download()
    faces.free()
    wf.free()
    np.testing.assert_array_equal(got[2], np.maximum(np.trunc(w), 1.0).astype(np.int32))
    if kind == "nomet":
        assert (got[2] == int(HUGE)).all()


# ---------------------------------------------------------------- 2. sizes, 3. empty rows

@pytest.mark.gpu
@pytest.mark.parametrize("m", [1, 2, 63, 64, 65, 255, 256, 257, 4097])
def test_sizes(ctx, dev, m):
    """the first m tetra, every link beyond them cut"""
    bg, _ = fixture()
    a = np.ascontiguousarray(cut(bg.adja, np.arange(bg.ne) < m)[:m])
    tv = np.ascontiguousarray(bg.tetv[:m])
    dt, da = up(ctx, tv, a)
    try:
        for kind in KINDS:
            got = graph(ctx, dev, kind, tetv=dt, adja=da)
            assert_graph(got, graph_ref(tv, a, kind))
            if m == 1:
                assert got[0].tolist() == [0, 0] and got[1].size == 0
    finally:
        dt.free()
        da.free()


@pytest.mark.gpu
def test_empty_rows(ctx, dev):
    """tetra 256..767 and every link to them cut: blocks 1 and 2 hold no entry"""
    bg, _ = fixture()
    keep = np.ones(bg.ne, bool)
    keep[256:768] = False
    a = cut(bg.adja, keep)
    (da,) = up(ctx, a)
    try:
        for kind in ("iso", "aniso", "noweights"):
            got = graph(ctx, dev, kind, adja=da)
            assert (np.diff(got[0])[256:768] == 0).all()
            assert_graph(got, graph_ref(bg.tetv, a, kind))
    finally:
        da.free()


# ---------------------------------------------------------------- 4. inputs, 5. unused tetra

@pytest.mark.gpu
@pytest.mark.parametrize("kind", ["aniso", "noweights"])
def test_inputs(ctx, dev, kind):
    """packed records, separate arrays and the adjacency built on the device give the same arrays"""
    bg, _ = fixture()
    want = graph_ref(bg.tetv, bg.adja, kind)
    assert_graph(graph(ctx, dev, kind), want)
    assert_graph(graph(ctx, dev, kind, tet8=dev["tet8"]), want)
    assert_graph(graph(ctx, dev, kind, adja=None), want)


@pytest.mark.gpu
def test_unused_tetra(ctx, dev):
    """rows with v[0] = 0, their links removed on both sides, are empty rows"""
    bg, _ = fixture()
    keep = np.ones(bg.ne, bool)
    keep[[0, 300, 5999]] = False
    a = cut(bg.adja, keep)
    tv = np.array(bg.tetv)
    tv[~keep, 0] = 0
    dt, da, d8 = up(ctx, tv, a, pack_tet8(tv, a))
    try:
        for kind in ("iso", "aniso", "nomet", "noweights"):
            want = graph_ref(tv, a, kind)
            assert want[0][301] == want[0][300]
            assert_graph(graph(ctx, dev, kind, tetv=dt, adja=da), want)
            assert_graph(graph(ctx, dev, kind, tet8=d8), want)
    finally:
        for d in (dt, da, d8):
            d.free()


# ---------------------------------------------------------------- 6. errors

def raw(ctx, dev, kind, cap, tetv=None, adja=None, np_=None):
    """the C call with sentinel-filled outputs of 22800 rows: (ok, nadjncy, xadj, adjncy, adjwgt, message)"""
    bg, _ = fixture()
    tetv = tetv or dev["tetv"]
    ne = tetv.shape[0]
    x, a, w = up(ctx, np.full(ne + 1, SENT, np.int32), np.full(22800, SENT, np.int32), np.full(22800, SENT, np.int32))
    n = ctypes.c_int64(-1)
    met = dev[kind]
    ok = ctx.lib.pmmg_hip_metis_graph(ctx.h, bg.np if np_ is None else np_, ctypes.c_void_p(dev["xyz"].ptr), ne,
                                      ctypes.c_void_p(tetv.ptr), ctypes.c_void_p((adja or dev["adja"]).ptr), None,
                                      0 if met is None else met.shape[1], None if met is None else ctypes.c_void_p(met.ptr),
                                      cap, ctypes.byref(n), ctypes.c_void_p(x.ptr), ctypes.c_void_p(a.ptr),
                                      ctypes.c_void_p(w.ptr) if kind != "noweights" else None)
    out = (ok, n.value, x.download(), a.download(), w.download(), ctx.error())
    for d in (x, a, w):
        d.free()
    return out


@pytest.mark.gpu
@pytest.mark.parametrize("kind", ["iso", "noweights"])
def test_cap_too_small(ctx, dev, kind):
    bg, _ = fixture()
    want = graph_ref(bg.tetv, bg.adja, kind)
    ok, n, x, a, w, msg = raw(ctx, dev, kind, 22800 - 1)
    assert ok == 0 and n == 22800 and "cap" in msg
    np.testing.assert_array_equal(x, want[0])
    assert (a == SENT).all() and (w == SENT).all()
    ok, n, x, a, w, _ = raw(ctx, dev, kind, 22800)
    assert ok == 1 and n == 22800
    np.testing.assert_array_equal(a, want[1])
    assert (w == SENT).all() if kind == "noweights" else (w == want[2]).all()


@pytest.mark.gpu
@pytest.mark.parametrize("where", [(0, 1), (5999, 3), (2571, 0)])
@pytest.mark.parametrize("value", ["4ne+4", "3", "-8", "2^31-1"])
def test_bad_link(ctx, dev, where, value):
    bg, _ = fixture()
    a = np.array(bg.adja)
    a[where] = {"4ne+4": 4 * bg.ne + 4, "3": 3, "-8": -8, "2^31-1": 2**31 - 1}[value]
    (da,) = up(ctx, a)
    try:
        for kind in ("aniso", "noweights"):
            ok, _, _, adj, w, msg = raw(ctx, dev, kind, 22800, adja=da)
            assert ok == 0 and "adja" in msg
            assert (adj == SENT).all() and (w == SENT).all()
    finally:
        da.free()


@pytest.mark.gpu
@pytest.mark.parametrize("value", ["np+1", "0", "-3", "2^31-1"])
def test_bad_vertex(ctx, dev, value):
    """with weights a vertex id outside [1, np] is refused before any coordinate is read; without weights
    the vertices are not looked at"""
    bg, _ = fixture()
    tv = np.array(bg.tetv)
    tv[4100, 2] = {"np+1": bg.np + 1, "0": 0, "-3": -3, "2^31-1": 2**31 - 1}[value]
    (dt,) = up(ctx, tv)
    try:
        for kind in ("iso", "aniso", "nomet"):
            ok, _, _, adj, w, msg = raw(ctx, dev, kind, 22800, tetv=dt)
            assert ok == 0 and "vertex id" in msg
            assert (adj == SENT).all() and (w == SENT).all()
        ok, n, x, adj, _, _ = raw(ctx, dev, "noweights", 22800, tetv=dt)
        want = graph_ref(bg.tetv, bg.adja, "noweights")
        assert ok == 1 and n == 22800
        np.testing.assert_array_equal(adj, want[1])
    finally:
        dt.free()


@pytest.mark.gpu
def test_link_to_unused_tetra(ctx, dev):
    """the reference requires a packed mesh: a link that points to an unused row is an error"""
    bg, _ = fixture()
    tv = np.array(bg.tetv)
    tv[300, 0] = 0
    (dt,) = up(ctx, tv)
    try:
        for kind in ("iso", "noweights"):
            ok, _, _, adj, w, msg = raw(ctx, dev, kind, 22800, tetv=dt)
            assert ok == 0 and "unused" in msg
            assert (adj == SENT).all() and (w == SENT).all()
    finally:
        dt.free()


@pytest.mark.gpu
def test_invalid_arguments(ctx, dev):
    bg, _ = fixture()
    n = ctypes.c_int64(0)
    x = ctx.empty((bg.ne + 1,), np.int32)
    p = lambda d: ctypes.c_void_p(d.ptr)
    call = ctx.lib.pmmg_hip_metis_graph
    # 2^29 tetra, a negative cap, weights with an unknown metric size, a misaligned tetra array
    assert call(ctx.h, bg.np, p(dev["xyz"]), 1 << 29, p(dev["tetv"]), p(dev["adja"]), None, 0, None, 0,
                ctypes.byref(n), p(x), None, None) == 0
    assert "2^29" in ctx.error()
    assert call(ctx.h, bg.np, p(dev["xyz"]), bg.ne, p(dev["tetv"]), p(dev["adja"]), None, 0, None, -1,
                ctypes.byref(n), p(x), None, None) == 0
    assert call(ctx.h, bg.np, p(dev["xyz"]), bg.ne, p(dev["tetv"]), p(dev["adja"]), None, 3, p(dev["iso"]), 0,
                ctypes.byref(n), p(x), None, p(x)) == 0
    assert call(ctx.h, bg.np, p(dev["xyz"]), bg.ne - 1, ctypes.c_void_p(dev["tetv"].ptr + 4), p(dev["adja"]), None, 0,
                None, 0, ctypes.byref(n), p(x), None, None) == 0
    assert "aligned" in ctx.error()
    x.free()


# ---------------------------------------------------------------- 7. determinism and bounds

def guarded(ctx, n, shift):
    """n int32 rows of SENT inside a device buffer with GUARD + shift bytes of FILL before and GUARD after"""
    raw_ = np.full(GUARD + shift + 4 * n + GUARD, FILL, np.uint8)
    raw_[GUARD + shift:GUARD + shift + 4 * n] = np.full(n, SENT, np.int32).view(np.uint8)
    buf = ctx.upload(raw_)
    return buf, DeviceArray(buf.ptr + GUARD + shift, 4 * n, (n,), np.dtype(np.int32), ctx)


def unguard(buf, n, shift):
    raw_ = buf.download()
    assert (raw_[:GUARD + shift] == FILL).all() and (raw_[GUARD + shift + 4 * n:] == FILL).all()
    return raw_[GUARD + shift:GUARD + shift + 4 * n].copy().view(np.int32)


@pytest.mark.gpu
@pytest.mark.parametrize("shift", [0, 4, 8, 12])
@pytest.mark.parametrize("kind", ["aniso", "noweights"])
def test_deterministic_and_in_bounds(ctx, dev, kind, shift):
    """two calls give the same bytes; 256 guard bytes around every output stay untouched, at every 4-byte
    position of the outputs within a 16-byte line; rows of adjncy / adjwgt beyond the count keep their fill"""
    bg, _ = fixture()
    want = graph_ref(bg.tetv, bg.adja, kind)
    extra = 5
    runs = []
    for _ in range(2):
        bufs = [guarded(ctx, bg.ne + 1, shift), guarded(ctx, 22800 + extra, shift),
                guarded(ctx, 22800 + extra, (shift + 4) % 16)]
        out = tuple(v for _, v in bufs)
        ctx.metis_graph(dev["xyz"], dev["tetv"], adja=dev["adja"], met=dev["aniso"], weights=kind != "noweights",
                        cap=22800 + extra, out=out)
        got = [unguard(bufs[0][0], bg.ne + 1, shift), unguard(bufs[1][0], 22800 + extra, shift),
               unguard(bufs[2][0], 22800 + extra, (shift + 4) % 16)]
        for b, _ in bufs:
            b.free()
        runs.append(got)
    for a, b in zip(*runs):
        assert a.tobytes() == b.tobytes()
    x, a, w = runs[0]
    np.testing.assert_array_equal(x, want[0])
    np.testing.assert_array_equal(a[:22800], want[1])
    assert (a[22800:] == SENT).all() and (w[22800:] == SENT).all()
    if kind == "noweights":
        assert (w == SENT).all()
    else:
        np.testing.assert_array_equal(w[:22800], want[2])


# ---------------------------------------------------------------- 8. history

@pytest.mark.gpu
def test_transfer_does_not_see_the_graph_scratch():
    """locate_interp after a metis_graph call (with a device-built adjacency) and release_scratch equals the
    same call on a fresh context bit for bit, hit kinds included"""
    bg, mets = fixture()
    case = make_case(kind=synth.CUBE, n_old=6, n_new=7, with_ref=False)
    fresh = run_gpu(case)
    with TransferContext(0) as c:
        d = [c.upload(a) for a in (bg.xyz, bg.tetv, mets["aniso"])]
        x, a, w = c.metis_graph(d[0], d[1], met=d[2])
        assert x.download()[-1] == 22800
        c.release_scratch()
        after = run_gpu(case, ctx=c)
        again = c.metis_graph(d[0], d[1], met=d[2])  # (the scratch comes back on demand)
        np.testing.assert_array_equal(again[2].download(), w.download())
    same_outputs(fresh, after)


# ---------------------------------------------------------------- 9. host layer

@pytest.mark.gpu
@pytest.mark.parametrize("with_adja", [True, False])
@pytest.mark.parametrize("kind", KINDS)
def test_host_layer(ctx, kind, with_adja):
    bg, mets = fixture()
    want = graph_ref(bg.tetv, bg.adja, kind)
    lib = _native.host_lib()
    P = ctypes.POINTER(ctypes.c_int)
    x, a, w, n = P(), P(), P(), ctypes.c_int64(-1)
    met = mets[kind]
    vp = lambda arr: None if arr is None else arr.ctypes.data_as(ctypes.c_void_p)
    ok = lib.pmmg_graph_mesh_elts2metis(ctx.h, bg.np, vp(bg.xyz), bg.ne, vp(bg.tetv), vp(bg.adja) if with_adja else None,
                                        0 if met is None else met.shape[1], vp(met), int(kind != "noweights"),
                                        ctypes.byref(x), ctypes.byref(a), ctypes.byref(w), ctypes.byref(n))
    assert ok == 1, ctx.error()
    try:
        assert n.value == 22800
        got = (np.ctypeslib.as_array(x, (bg.ne + 1,)).copy(), np.ctypeslib.as_array(a, (n.value,)).copy(),
               np.ctypeslib.as_array(w, (n.value,)).copy() if kind != "noweights" else None)
        assert bool(w) == (kind != "noweights")
        assert_graph(got, want)
    finally:
        for q in (x, a, w):
            lib.pmmg_host_free(q)
