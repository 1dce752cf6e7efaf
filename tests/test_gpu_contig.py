"""pmmg_hip_part_subgroups and pmmg_hip_fix_contiguity against the restatement
of tests/contig_ref.py, exactly (runs on the MI355X).

tests/test_contig_ref_host.py shows, on the CPU, that the restatement used
here (the statement of include/parmmg_hip.h) equals the reference's flagged
loop under the module's choice of the neighbouring colour, and that on the
lattice-numbered fixtures this choice equals the reference's own: there the
comparison is one against the reference.

Every call of this file goes through sub() or fix(), which put 256 guard
bytes around every output, device or host, and hold the labelling to its
proven bound: rounds <= 2 ceil(log2 ne) + 1 (contig_ref.round_bound, DESIGN.md
§11; a plain label propagation needs thousands of rounds on the scrambled
paths).  The trees of contig_ref.TREES are the scheme's adversarial inputs:
they need more than ceil(log2 ne) + 1 rounds, 56 tetra more than
ceil(log2 ne) + 2.  A round on the device reads only the labels of its start,
so its round count is that of contig_ref.hook_rounds, the round-by-round
simulation, exactly: asserted wherever sub() is given the host arrays."""
import ctypes
import functools

import numpy as np
import pytest

import contig_ref as R
from parity import make_case, run_gpu, same_outputs
from parmmg_amd import _native, synth
from parmmg_amd.transfer import DeviceArray, TransferContext, pack_tet8
from test_metis_graph import cut, fixture

GUARD = 256
FILL = 0xA5
SENT = -7
P = lambda d: None if d is None else ctypes.c_void_p(d.ptr)


@pytest.fixture(scope="module")
def ctx():
    with TransferContext(0) as c:
        yield c


def guarded(ctx, values):
    """int32 values inside a device buffer with GUARD bytes of FILL on both sides: (buffer, view)"""
    values = np.ascontiguousarray(values, np.int32)
    raw = np.full(2 * GUARD + 4 * values.size, FILL, np.uint8)
    raw[GUARD:GUARD + 4 * values.size] = values.view(np.uint8)
    buf = ctx.upload(raw)
    return buf, DeviceArray(buf.ptr + GUARD, 4 * values.size, (values.size,), np.dtype(np.int32), ctx)


def unguard(buf, n):
    raw = buf.download()
    buf.free()
    assert (raw[:GUARD] == FILL).all() and (raw[GUARD + 4 * n:] == FILL).all(), "a write outside a device output"
    return raw[GUARD:GUARD + 4 * n].copy().view(np.int32)


def host_guarded(n):
    """n int32 of SENT between two guard zones of 64 words on the host: (whole, pointer to the payload)"""
    whole = np.full(n + 128, 0x5A5A5A5A, np.int32)
    whole[64:64 + n] = SENT
    return whole, ctypes.c_void_p(whole.ctypes.data + 256)


def host_unguard(whole, n):
    assert (whole[:64] == 0x5A5A5A5A).all() and (whole[64 + n:] == 0x5A5A5A5A).all(), "a write outside a host output"
    return whole[64:64 + n].copy()


bound = R.round_bound


def sub(ctx, ne, tetv=None, adja=None, tet8=None, part=None, ncolor=1, cap=None, want_ok=True, sim=None):
    """the C call with guarded outputs: dict(ok, head, flag, ncomp, sub [cap, 4], nsub, rounds, msg).  sim = (adja,
    part | None) on the host: the call's rounds must be those of the round-by-round simulation, exactly (a round
    on the device reads only the labels of its start)"""
    cap = ne if cap is None else cap
    hb, head = guarded(ctx, np.full(ne, SENT))
    fb, flag = guarded(ctx, np.full(ne, SENT))
    ncomp_w, ncomp_p = host_guarded(ncolor)
    table_w, table_p = host_guarded(4 * cap)
    n, rounds = ctypes.c_int64(-1), ctypes.c_int(-1)
    ok = ctx.lib.pmmg_hip_part_subgroups(ctx.h, ne, P(tetv), P(adja), P(tet8), P(part), ncolor, P(head), P(flag),
                                         ctypes.cast(ncomp_p, ctypes.POINTER(ctypes.c_int)), cap,
                                         ctypes.cast(table_p, ctypes.POINTER(_native.HipSubgroup)), ctypes.byref(n),
                                         ctypes.byref(rounds))
    out = dict(ok=ok, head=unguard(hb, ne), flag=unguard(fb, ne), ncomp=host_unguard(ncomp_w, ncolor),
               sub=host_unguard(table_w, 4 * cap).reshape(-1, 4), nsub=n.value, rounds=rounds.value, msg=ctx.error())
    if want_ok:
        assert ok == 1, out["msg"]
        print("ne", ne, "subgroups", out["nsub"], "rounds", out["rounds"], "bound", bound(ne), "passes",
              ctx.lib.pmmg_hip_contig_passes(ctx.h))
        assert 1 <= out["rounds"] <= bound(ne)
        if sim is not None:
            assert out["rounds"] == R.hook_rounds(*sim)[0]
    return out


def fix(ctx, ne, part_values, ncolor, tetv=None, adja=None, tet8=None, want_ok=True):
    """the C call on a guarded copy of part: dict(ok, part, nmoved, nmerged, nstuck, msg)"""
    pb, part = guarded(ctx, part_values)
    nmoved, nmerged, nstuck = ctypes.c_int64(-1), ctypes.c_int(-1), ctypes.c_int(-1)
    ok = ctx.lib.pmmg_hip_fix_contiguity(ctx.h, ne, P(tetv), P(adja), P(tet8), P(part), ncolor, ctypes.byref(nmoved),
                                         ctypes.byref(nmerged), ctypes.byref(nstuck))
    out = dict(ok=ok, part=unguard(pb, ne), nmoved=nmoved.value, nmerged=nmerged.value, nstuck=nstuck.value,
               msg=ctx.error())
    if want_ok:
        assert ok == 1, out["msg"]
    return out


def up(ctx, *arrays):
    return [None if a is None else ctx.upload(np.ascontiguousarray(a)) for a in arrays]


def free(*devs):
    for d in devs:
        if d is not None:
            d.free()


@functools.lru_cache(maxsize=None)
def reference(name):
    """(case dict, subgroups(), fix_free()) of a fixture of contig_ref, computed once"""
    g = R.mesh_case(*name) if isinstance(name, tuple) else R.graph_case(name)
    ne = g["adja"].shape[0]
    part = g["part"] if g["part"] is not None else np.zeros(ne, np.int32)
    return g, R.subgroups(g["adja"], g["part"], g["ncolor"]), R.fix_free(g["adja"], part, g["ncolor"])


def assert_sub(got, want, used=None):
    head, flag, ncomp, table = want
    np.testing.assert_array_equal(got["head"], head)
    np.testing.assert_array_equal(got["flag"], flag)
    np.testing.assert_array_equal(got["ncomp"], ncomp)
    assert got["nsub"] == table.shape[0]
    np.testing.assert_array_equal(got["sub"][:got["nsub"]], table)
    assert (got["sub"][got["nsub"]:] == SENT).all()


def assert_fix(got, want):
    np.testing.assert_array_equal(got["part"], want["part"])
    assert (got["nmoved"], got["nmerged"], got["nstuck"]) == (want["nmoved"], want["nmerged"], want["nstuck"])


# ---------------------------------------------------------------- 1. the fixtures, on every input layout

@pytest.mark.gpu
@pytest.mark.parametrize("name", R.MESH_CASES, ids=str)
def test_mesh_fixtures(ctx, name):
    g, want_sub, want_fix = reference(name)
    ne, ncolor = g["adja"].shape[0], g["ncolor"]
    tetv, adja, tet8, part = up(ctx, g["tetv"], g["adja"], pack_tet8(g["tetv"], g["adja"]), g["part"])
    after = R.subgroups(g["adja"], want_fix["part"], ncolor)[2]
    try:
        for kw in (dict(tet8=tet8), dict(tetv=tetv, adja=adja), dict(tetv=tetv)):  # the last: built on the device
            assert_sub(sub(ctx, ne, part=part, ncolor=ncolor, sim=(g["adja"], g["part"]), **kw), want_sub)
            got = fix(ctx, ne, g["part"], ncolor, **kw)
            assert_fix(got, want_fix)
            (fixed,) = up(ctx, got["part"])
            again = sub(ctx, ne, part=fixed, ncolor=ncolor, sim=(g["adja"], got["part"]), **kw)
            free(fixed)
            np.testing.assert_array_equal(again["ncomp"], after)
            assert (again["ncomp"][after <= 1] <= 1).all()
        if not name[1]:  # lattice numbering: the reference's own rule gives the same partition
            np.testing.assert_array_equal(got["part"], R.fix_flagged(g["adja"], g["part"], ncolor, "bfs")["part"])
    finally:
        free(tetv, adja, tet8, part)


@pytest.mark.gpu
@pytest.mark.parametrize("name", R.SMALL_GRAPHS + R.PATH_GRAPHS + R.TREE_GRAPHS)
def test_graphs(ctx, name):
    """pure adjacency: no vertices, adja written directly"""
    g, want_sub, want_fix = reference(name)
    ne, ncolor = g["adja"].shape[0], g["ncolor"]
    adja, part = up(ctx, g["adja"], g["part"])
    try:
        got = sub(ctx, ne, adja=adja, part=part, ncolor=ncolor, sim=(g["adja"], g["part"]))
        assert_sub(got, want_sub)
        if name in R.PATH_GRAPHS + R.TREE_GRAPHS:
            print(name, "rounds", got["rounds"])
        if name in R.TREE_GRAPHS:
            assert got["rounds"] == R.TREE_ROUNDS[name] > int(np.ceil(np.log2(ne))) + 1
        if name == "scrambled65537_one":
            assert got["rounds"] == 11 and got["nsub"] == 1 and got["sub"][0].tolist() == [0, 1, 65537, 0]
        if name in R.TREE_GRAPHS:
            assert got["nsub"] == 1 and got["sub"][0].tolist() == [0, 1, ne, 0]
        if g["part"] is not None:
            assert_fix(fix(ctx, ne, g["part"], ncolor, adja=adja), want_fix)
        if name == "path7":
            assert want_fix["part"].tolist() == [0, 0, 0, 1, 1, 1, 1]
            assert R.fix_oneshot(g["adja"], g["part"], ncolor)["part"].tolist() != want_fix["part"].tolist()
        if name == "stuck":
            assert (want_fix["nmerged"], want_fix["nstuck"]) == (0, 1)
    finally:
        free(adja, part)


# ---------------------------------------------------------------- 2. sizes, unused tetra

@pytest.mark.gpu
@pytest.mark.parametrize("m", [1, 2, 63, 64, 65, 255, 256, 257, 4097])
def test_sizes(ctx, m):
    """the first m tetra of the lattice, every link beyond them cut: one colour and case (a)'s colours"""
    bg, _ = fixture()
    a = np.ascontiguousarray(cut(bg.adja, np.arange(bg.ne) < m)[:m])
    tv = np.ascontiguousarray(bg.tetv[:m])
    colours = np.ascontiguousarray(R.colours("a")[0][:m])
    tetv, adja, tet8, part = up(ctx, tv, a, pack_tet8(tv, a), colours)
    try:
        for kw in (dict(tetv=tetv, adja=adja), dict(tet8=tet8), dict(adja=adja)):
            assert_sub(sub(ctx, m, sim=(a, None), **kw), R.subgroups(a, None, 1))
            assert_sub(sub(ctx, m, part=part, ncolor=4, sim=(a, colours), **kw), R.subgroups(a, colours, 4))
            assert_fix(fix(ctx, m, colours, 4, **kw), R.fix_free(a, colours, 4))
    finally:
        free(tetv, adja, tet8, part)


@pytest.mark.gpu
@pytest.mark.parametrize("scrambled", [False, True])
def test_unused_band(ctx, scrambled):
    """512 unused tetra (v[0] = 0, every link to them cut): head / flag 0 there, their part untouched by the fix"""
    g = R.mesh_case("a", scrambled)
    ne, ncolor = 6000, g["ncolor"]
    used = np.ones(ne, bool)
    used[256:768] = False
    a = cut(g["adja"], used)
    tv = np.array(g["tetv"])
    tv[~used, 0] = 0
    colours = np.array(g["part"])
    colours[~used] = 1 << 20  # (neither read nor written: not a colour)
    tetv, adja, tet8, part = up(ctx, tv, a, pack_tet8(tv, a), colours)
    want_sub, want_fix = R.subgroups(a, colours, ncolor, used), R.fix_free(a, colours, ncolor, used)
    assert (want_sub[0][~used] == 0).all() and (want_fix["part"][~used] == 1 << 20).all() and want_fix["nmerged"] > 0
    try:
        for kw in (dict(tetv=tetv, adja=adja), dict(tet8=tet8)):
            got = sub(ctx, ne, part=part, ncolor=ncolor, sim=(a, colours), **kw)  # (an unused tetra has no link)
            assert_sub(got, want_sub)
            assert (got["head"][~used] == 0).all() and (got["flag"][~used] == 0).all()
            assert_fix(fix(ctx, ne, colours, ncolor, **kw), want_fix)
            one = sub(ctx, ne, **kw)  # the group check: part NULL
            assert_sub(one, R.subgroups(a, None, 1, used))
    finally:
        free(tetv, adja, tet8, part)


# ---------------------------------------------------------------- 3. refusals

@pytest.mark.gpu
@pytest.mark.parametrize("what", ["link 4ne+4", "link 3", "link -8", "link to unused", "part ncolor", "part -1",
                                  "ncolor 2 without part", "2^29"])
def test_refusals(ctx, what):
    """each returns 0 with a message and nothing written to part, head, flag or the table"""
    g = R.mesh_case("a", False)
    ne, ncolor = 6000, g["ncolor"]
    tv, a, colours = np.array(g["tetv"]), np.array(g["adja"]), np.array(g["part"])
    word = "adja"
    if what.startswith("link "):
        if what == "link to unused":
            tv[300, 0] = 0
            word = "unused"
        else:
            a[2571, 2] = {"4ne+4": 4 * ne + 4, "3": 3, "-8": -8}[what[5:]]
    elif what.startswith("part "):
        colours[4100] = ncolor if what == "part ncolor" else -1
        word = "part"
    tetv, adja, part = up(ctx, tv, a, colours)
    n = ne
    if what == "ncolor 2 without part":
        free(part)
        part, ncolor, word = None, 2, "ncolor"
    if what == "2^29":
        n, word = 1 << 29, "2^29"
    try:
        # (the outputs are sized for the real mesh: a refused call writes to none of them)
        hb, head = guarded(ctx, np.full(ne, SENT))
        ncomp_w, ncomp_p = host_guarded(ncolor)
        table_w, table_p = host_guarded(4 * 64)
        cnt = ctypes.c_int64(-1)
        ok = ctx.lib.pmmg_hip_part_subgroups(ctx.h, n, P(tetv), P(adja), None, P(part), ncolor, P(head), None,
                                             ctypes.cast(ncomp_p, ctypes.POINTER(ctypes.c_int)), 64,
                                             ctypes.cast(table_p, ctypes.POINTER(_native.HipSubgroup)),
                                             ctypes.byref(cnt), None)
        assert ok == 0 and word in ctx.error(), ctx.error()
        assert (unguard(hb, ne) == SENT).all() and (host_unguard(table_w, 4 * 64) == SENT).all()
        host_unguard(ncomp_w, ncolor)
        if part is not None:
            got = fix(ctx, n, colours, ncolor, tetv=tetv, adja=adja, want_ok=False) if n == ne else None
            if got is None:  # 2^29: the guarded copy has the real size
                pb, pv = guarded(ctx, colours)
                z = ctypes.c_int64(0), ctypes.c_int(0), ctypes.c_int(0)
                ok = ctx.lib.pmmg_hip_fix_contiguity(ctx.h, n, P(tetv), P(adja), None, P(pv), ncolor,
                                                     ctypes.byref(z[0]), ctypes.byref(z[1]), ctypes.byref(z[2]))
                got = dict(ok=ok, part=unguard(pb, ne), msg=ctx.error())
            assert got["ok"] == 0 and word in got["msg"], got["msg"]
            np.testing.assert_array_equal(got["part"], colours)
    finally:
        free(tetv, adja, part)


@pytest.mark.gpu
def test_cap_too_small(ctx):
    g, want_sub, _ = reference(("b", True))
    ne, ncolor, nsub = 6000, g["ncolor"], want_sub[3].shape[0]
    adja, part = up(ctx, g["adja"], g["part"])
    try:
        for cap in (0, nsub - 1):
            got = sub(ctx, ne, adja=adja, part=part, ncolor=ncolor, cap=cap, want_ok=False)
            assert got["ok"] == 0 and "cap" in got["msg"] and got["nsub"] == nsub
            np.testing.assert_array_equal(got["ncomp"], want_sub[2])
            assert (got["sub"] == SENT).all()
        assert_sub(sub(ctx, ne, adja=adja, part=part, ncolor=ncolor, cap=nsub), want_sub)
    finally:
        free(adja, part)


# ---------------------------------------------------------------- 4. determinism, history

@pytest.mark.gpu
@pytest.mark.parametrize("name", [("c", True), "scrambled4097_bands"], ids=str)
def test_two_calls_are_byte_identical(ctx, name):
    g, _, _ = reference(name)
    ne, ncolor = g["adja"].shape[0], g["ncolor"]
    adja, part = up(ctx, g["adja"], g["part"])
    try:
        a, b = [sub(ctx, ne, adja=adja, part=part, ncolor=ncolor) for _ in range(2)]
        for k in ("head", "flag", "ncomp", "sub"):
            assert a[k].tobytes() == b[k].tobytes(), k
        assert (a["nsub"], a["rounds"]) == (b["nsub"], b["rounds"])
        fa, fb = [fix(ctx, ne, g["part"], ncolor, adja=adja) for _ in range(2)]
        assert fa["part"].tobytes() == fb["part"].tobytes()
        assert [fa[k] for k in ("nmoved", "nmerged", "nstuck")] == [fb[k] for k in ("nmoved", "nmerged", "nstuck")]
    finally:
        free(adja, part)


@pytest.mark.gpu
def test_call_history(ctx):
    """five calls of different ne on one context (the scratch grows, shrinks in use, is released once), each
    equal to the same call on a fresh context"""
    names = [("a", True), "scrambled4097_bands", "path7", "tree56", "scrambled65537_bands"]  # 6000, 4097, 7, 56, 65537
    assert len({reference(n)[0]["adja"].shape[0] for n in names}) == 5

    def both(c, name):
        g, _, _ = reference(name)
        ne, ncolor = g["adja"].shape[0], g["ncolor"]
        adja, part = up(c, g["adja"], g["part"])
        colours = g["part"] if g["part"] is not None else np.zeros(ne, np.int32)
        try:
            return sub(c, ne, adja=adja, part=part, ncolor=ncolor), fix(c, ne, colours, ncolor, adja=adja)
        finally:
            free(adja, part)

    for i, name in enumerate(names):
        if i == 3:
            ctx.release_scratch()
        s, f = both(ctx, name)
        with TransferContext(0) as fresh:
            s0, f0 = both(fresh, name)
        for k in ("head", "flag", "ncomp", "sub"):
            assert s[k].tobytes() == s0[k].tobytes(), (name, k)
        assert f["part"].tobytes() == f0["part"].tobytes() and f["nmoved"] == f0["nmoved"]
        _, want_sub, want_fix = reference(name)
        assert_sub(s, want_sub)
        assert_fix(f, want_fix)


@pytest.mark.gpu
def test_transfer_does_not_see_the_contiguity_scratch():
    """locate_interp before and after a contiguity call (adjacency built on the device), and again after
    release_scratch, gives the same outputs bit for bit"""
    g, want_sub, want_fix = reference(("b", False))
    case = make_case(kind=synth.CUBE, n_old=6, n_new=7, with_ref=False)
    with TransferContext(0) as c:
        before = run_gpu(case, ctx=c)
        tetv, part = up(c, g["tetv"], g["part"])
        assert_sub(sub(c, 6000, tetv=tetv, part=part, ncolor=g["ncolor"]), want_sub)
        assert_fix(fix(c, 6000, g["part"], g["ncolor"], tetv=tetv), want_fix)
        after = run_gpu(case, ctx=c)
        c.release_scratch()
        released = run_gpu(case, ctx=c)
        assert_sub(sub(c, 6000, tetv=tetv, part=part, ncolor=g["ncolor"]), want_sub)  # (the scratch comes back)
        free(tetv, part)
    same_outputs(before, after)
    same_outputs(before, released)


# ---------------------------------------------------------------- 5. Python front-end, host layer

@pytest.mark.gpu
def test_python_front_end(ctx):
    g, want_sub, want_fix = reference(("b", True))
    tetv, adja, part = up(ctx, g["tetv"], g["adja"], np.array(g["part"]))
    head, flag = ctx.empty((6000,), np.int32), ctx.empty((6000,), np.int32)
    try:
        out = ctx.part_subgroups(tetv, adja=adja, part=part, ncolor=g["ncolor"], head=head, flag=flag)
        np.testing.assert_array_equal(out["sub"], want_sub[3])
        np.testing.assert_array_equal(out["ncomp"], want_sub[2])
        np.testing.assert_array_equal(head.download(), want_sub[0])
        np.testing.assert_array_equal(flag.download(), want_sub[1])
        assert 1 <= out["rounds"] <= bound(6000) and out["passes"] >= 1
        one = ctx.part_subgroups(tetv)  # the group check, adjacency built on the device
        assert one["ncomp"].tolist() == [1] and one["sub"].tolist() == [[0, 1, 6000, 0]]
        res = ctx.fix_contiguity(tetv, part, g["ncolor"], adja=adja)
        np.testing.assert_array_equal(part.download(), want_fix["part"])
        assert (res["nmoved"], res["nmerged"], res["nstuck"]) == tuple(want_fix[k] for k in ("nmoved", "nmerged", "nstuck"))
        with pytest.raises(ValueError):
            ctx.part_subgroups(g["tetv"])
    finally:
        free(tetv, adja, part, head, flag)


@pytest.mark.gpu
@pytest.mark.parametrize("with_adja", [True, False])
def test_host_layer(ctx, with_adja):
    g, want_sub, want_fix = reference(("a", True))
    lib = _native.host_lib()
    vp = lambda arr: None if arr is None else arr.ctypes.data_as(ctypes.c_void_p)
    a = g["adja"] if with_adja else None
    ncomp = np.full(g["ncolor"], SENT, np.int32)
    ret = lib.pmmg_check_part_contiguity(ctx.h, 6000, vp(g["tetv"]), vp(a), vp(g["part"]), g["ncolor"], vp(ncomp))
    np.testing.assert_array_equal(ncomp, want_sub[2])
    assert ret == want_sub[2][-1]  # the reference returns the last colour's count
    one = np.full(1, SENT, np.int32)
    assert lib.pmmg_check_part_contiguity(ctx.h, 6000, vp(g["tetv"]), vp(a), None, 1, vp(one)) == 1 and one[0] == 1
    part = np.array(g["part"])
    assert lib.pmmg_fix_contiguity_split(ctx.h, 6000, vp(g["tetv"]), vp(a), g["ncolor"], vp(part)) == 1
    np.testing.assert_array_equal(part, want_fix["part"])
    bad = np.array(g["part"])
    bad[17] = g["ncolor"]
    keep = bad.copy()
    assert lib.pmmg_fix_contiguity_split(ctx.h, 6000, vp(g["tetv"]), vp(a), g["ncolor"], vp(bad)) == 0
    np.testing.assert_array_equal(bad, keep)
    assert lib.pmmg_check_part_contiguity(ctx.h, 6000, vp(g["tetv"]), vp(a), vp(bad), g["ncolor"], vp(ncomp)) == -1
