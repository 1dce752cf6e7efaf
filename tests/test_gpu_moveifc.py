"""pmmg_hip_ifc_seed, pmmg_hip_ifc_layers and pmmg_hip_remap_colors against
the restatements of tests/moveifc_ref.py, exactly (runs on the MI355X).

tests/test_moveifc_ref_host.py shows, on the CPU, that the definition the
device computes (ifc_par) equals the reference's transcribed loop (ifc_seq with
the module's side-point tie) on these fixtures.  Every call of this file goes
through seed() or layers(), which put 256 guard bytes around every device
output and guard words around every host output."""
import ctypes
import functools

import numpy as np
import pytest

import contig_ref as R
import moveifc_ref as M
from parity import make_case, run_gpu, same_outputs
from parmmg_amd import _native, synth
from parmmg_amd.transfer import DeviceArray, TransferContext, pack_tet8
from test_gpu_contig import FILL, GUARD, SENT, P, free, guarded, host_guarded, host_unguard, unguard, up
from test_metis_graph import cut
from test_moveifc_ref_host import brake_fixture, nelem_of, seq, set_points

CI = ctypes.POINTER(ctypes.c_int)


@pytest.fixture(scope="module")
def ctx():
    with TransferContext(0) as c:
        yield c


def guarded_bytes(ctx, values):
    values = np.ascontiguousarray(values, np.uint8)
    raw = np.full(2 * GUARD + values.size, FILL, np.uint8)
    raw[GUARD:GUARD + values.size] = values
    buf = ctx.upload(raw)
    return buf, DeviceArray(buf.ptr + GUARD, values.size, (values.size,), np.dtype(np.uint8), ctx)


def unguard_bytes(buf, n):
    raw = buf.download()
    buf.free()
    assert (raw[:GUARD] == FILL).all() and (raw[GUARD + n:] == FILL).all(), "a write outside a device output"
    return raw[GUARD:GUARD + n].copy()


def mesh_args(ctx, tetv, layout):
    """(tetv device or None, tet8 device or None)"""
    tetv = np.ascontiguousarray(tetv, np.int32)
    if layout == "tet8":
        return None, ctx.upload(pack_tet8(tetv, np.zeros_like(tetv)))
    return ctx.upload(tetv), None


def seed(ctx, tetv, np_, mark, w, layout="tetv", ne=None, want_ok=True, dev=None):
    """the C call with guarded outputs: dict(ok, color, front, msg)"""
    dt, d8 = dev if dev is not None else mesh_args(ctx, tetv, layout)
    (dm,) = up(ctx, np.asarray(mark, np.int32))
    w = np.ascontiguousarray(w, np.int32)
    cb, color = guarded(ctx, np.full(np_, SENT))
    fb, front = guarded_bytes(ctx, np.full(np_, 0x77))
    ok = ctx.lib.pmmg_hip_ifc_seed(ctx.h, np_, len(tetv) if ne is None else ne, P(dt), P(d8), P(dm), w.size,
                                   w.ctypes.data_as(ctypes.c_void_p), P(color), P(front))
    out = dict(ok=ok, color=unguard(cb, np_), front=unguard_bytes(fb, np_), msg=ctx.error())
    free(dm, *(() if dev is not None else (dt, d8)))
    if want_ok:
        assert ok == 1, out["msg"]
    return out


def layers(ctx, tetv, np_, mark, w, nelem, nemin, nl, layout="tetv", color=None, front=None, set_pt=None,
           set_color=None, ne=None, want_ok=True, dev=None):
    """the C call on guarded copies: dict(ok, mark, color, front, nelem, moved, done, blocked, msg); without a
    state (color, front) the seed is taken first"""
    if color is None:
        s = seed(ctx, tetv, np_, mark, w, layout, dev=dev)
        color, front = s["color"], s["front"]
    dt, d8 = dev if dev is not None else mesh_args(ctx, tetv, layout)
    w = np.ascontiguousarray(w, np.int32)
    ncolor = w.size
    mb, dmark = guarded(ctx, mark)
    cb, dcolor = guarded(ctx, color)
    fb, dfront = guarded_bytes(ctx, front)
    dsp, dsc = up(ctx, None if set_pt is None else np.asarray(set_pt, np.int32),
                  None if set_color is None else np.asarray(set_color, np.int32))
    ne_w, ne_p = host_guarded(ncolor)
    ne_w[64:64 + ncolor] = nelem
    nemin = np.ascontiguousarray(nemin, np.int32)
    mv_w, mv_p = host_guarded(max(nl, 1))
    st_w, st_p = host_guarded(2)
    ok = ctx.lib.pmmg_hip_ifc_layers(ctx.h, np_, len(tetv) if ne is None else ne, P(dt), P(d8), P(dmark), ncolor,
                                     w.ctypes.data_as(ctypes.c_void_p), ne_p, nemin.ctypes.data_as(ctypes.c_void_p),
                                     P(dcolor), P(dfront), 0 if set_pt is None else len(set_pt), P(dsp), P(dsc), nl,
                                     ctypes.cast(st_p, CI), ctypes.cast(ctypes.c_void_p(st_p.value + 4), CI), mv_p)
    st = host_unguard(st_w, 2)
    out = dict(ok=ok, mark=unguard(mb, len(mark)), color=unguard(cb, np_), front=unguard_bytes(fb, np_),
               nelem=host_unguard(ne_w, ncolor), moved=host_unguard(mv_w, max(nl, 1))[:nl], done=int(st[0]),
               blocked=int(st[1]), msg=ctx.error())
    free(dsp, dsc, *(() if dev is not None else (dt, d8)))
    if want_ok:
        assert ok == 1, out["msg"]
    return out


def assert_state(got, want, what=""):
    """got: a layers() result; want: a layer record of moveifc_ref"""
    for key in ("mark", "color", "front"):
        np.testing.assert_array_equal(got[key], want[key], err_msg=f"{key} {what}")
    if "nelem" in want:
        np.testing.assert_array_equal(got["nelem"], want["nelem"], err_msg=f"nelem {what}")


def case_inputs(case, wkind, local):
    g = R.mesh_case(*case)
    w = M.weight_table(wkind, g["part"], g["ncolor"])
    nelem = nelem_of(g, local)
    return g, w, nelem, M.nemin_of(nelem)


# ---------------------------------------------------------------- 1. exact against the transcribed loop

@pytest.mark.gpu
@pytest.mark.parametrize("wkind", M.WEIGHTS)
@pytest.mark.parametrize("case", R.MESH_CASES, ids=str)
def test_mesh_fixtures(ctx, case, wkind):
    g, w, nelem, nemin = case_inputs(case, wkind, False)
    tetv, part, np_ = g["tetv"], g["part"], g["np"]
    want = seq(case, wkind, False, False)
    st = M.seed_seq(tetv, part, w, np_)
    for layout in ("tetv", "tet8"):
        s = seed(ctx, tetv, np_, part, w, layout)
        np.testing.assert_array_equal(s["color"], st["tmp"][1:])
        np.testing.assert_array_equal(s["front"], [f == st["bf"] for f in st["flag"][1:]])
        for nl in (1, 2, 4):
            got = layers(ctx, tetv, np_, part, w, nelem, nemin, nl, layout)
            assert (got["done"], got["blocked"]) == (nl, 0)
            assert_state(got, want[nl - 1], f"{layout} after {nl} layers")
            assert got["moved"].tolist() == [l["moved"] for l in want[:nl]]
    # one call of two layers is two calls of one
    one = layers(ctx, tetv, np_, part, w, nelem, nemin, 1)
    two = layers(ctx, tetv, np_, one["mark"], w, one["nelem"], nemin, 1, color=one["color"], front=one["front"])
    assert_state(two, want[1], "two calls")
    assert two["moved"].tolist() == [want[1]["moved"]]
    # the brake's counts: every colour local, compared up to the layer the definition blocks
    g, w, nelem, nemin = case_inputs(case, wkind, True)
    want = seq(case, wkind, False, True)
    got = layers(ctx, tetv, np_, part, w, nelem, nemin, 4, "tet8")
    print(case, wkind, "local: layers done", got["done"], "blocked", got["blocked"], "moved", got["moved"])
    assert all(l["abandoned"] == 0 for l in want[:got["done"]])
    if got["blocked"]:
        assert want[got["done"]]["abandoned"] > 0 and (got["moved"][got["done"]:] == 0).all()
    if got["done"]:
        assert_state(got, want[got["done"] - 1], "local")
    else:
        np.testing.assert_array_equal(got["mark"], part)
        np.testing.assert_array_equal(got["nelem"], nelem)


@functools.lru_cache(maxsize=None)
def seq_set_without_colour(case, wkind):
    g, w, nelem, nemin = case_inputs(case, wkind, False)
    return M.ifc_seq(g["tetv"], g["adja"], g["part"], w, nelem, nemin, g["np"], 2, set_points(g)[0], None)


@pytest.mark.gpu
@pytest.mark.parametrize("wkind", M.WEIGHTS)
@pytest.mark.parametrize("case", R.MESH_CASES, ids=str)
def test_set_points(ctx, case, wkind):
    g, w, nelem, nemin = case_inputs(case, wkind, False)
    sp, sc = set_points(g)
    for colours, want in ((sc, seq(case, wkind, True, False)), (None, seq_set_without_colour(case, wkind))):
        got = layers(ctx, g["tetv"], g["np"], g["part"], w, nelem, nemin, 2, set_pt=sp, set_color=colours)
        assert (got["done"], got["blocked"]) == (2, 0)
        assert_state(got, want[1], "with set points")
        assert got["moved"].tolist() == [l["moved"] for l in want[:2]]


# ---------------------------------------------------------------- 2. size edges

@pytest.mark.gpu
@pytest.mark.parametrize("ne", [1, 63, 64, 65, 255, 256, 257])
def test_paths(ctx, ne):
    """paths of ne tetra in bands of 5 of 3 colours, two points beyond the mesh's own"""
    tetv, adja, np_ = M.path_mesh(ne)
    np_ += 2
    mark, w = M.bands(ne, 5, 3), np.array([3, 1, 2], np.int32)
    none = np.full(3, -1, np.int32)
    want = M.ifc_seq(tetv, adja, mark, w, none, none * 0, np_, 2)
    s = seed(ctx, tetv, np_, mark, w)
    assert s["color"][-2:].tolist() == [-1, -1] and s["front"][-2:].tolist() == [0, 0]
    got = layers(ctx, tetv, np_, mark, w, none, none * 0, 2)
    assert_state(got, want[1])
    assert got["moved"].tolist() == [l["moved"] for l in want] and got["color"][-2:].tolist() == [-1, -1]


@pytest.mark.gpu
def test_unused_tetra_never_change_and_never_influence(ctx):
    """runs of three unused tetra along a path of 257 (the pieces between them share no point, so every star stays
    face-connected), their marks outside the colours: the result is that of the mesh without them, their marks stay"""
    tetv, adja, np_ = M.path_mesh(257)
    tetv = tetv.copy()
    keep = ~np.isin(np.arange(257) % 12, (3, 4, 5))
    tetv[~keep] = 0
    adja = cut(adja, keep)
    assert M.stars_face_connected(tetv, adja)
    mark, w = M.bands(257, 5, 3), np.array([3, 1, 2], np.int32)
    mark[~keep] = 99
    none = np.full(3, -1, np.int32)
    want = M.ifc_seq(tetv, adja, mark, w, none, none * 0, np_, 2)
    got = layers(ctx, tetv, np_, mark, w, none, none * 0, 2)
    assert_state(got, want[1])
    assert (got["mark"][~keep] == 99).all() and got["moved"].sum() > 0
    part, ngrp = remap(ctx, tetv, got["mark"], 3, np.array([2, 0, 1], np.int32))
    want_part, want_n = M.remap(tetv, got["mark"], 3, np.array([2, 0, 1], np.int32))
    np.testing.assert_array_equal(part, want_part)
    assert ngrp == want_n


@pytest.mark.gpu
def test_one_colour_nothing_moves(ctx):
    g = R.mesh_case("a", False)
    mark, w, n = np.zeros(6000, np.int32), np.array([7], np.int32), np.array([6000], np.int32)
    s = seed(ctx, g["tetv"], g["np"], mark, w)
    assert (s["color"] == 0).all() and not s["front"].any()
    got = layers(ctx, g["tetv"], g["np"], mark, w, n, M.nemin_of(n), 2)
    assert (got["done"], got["blocked"], got["moved"].tolist()) == (2, 0, [0, 0])
    assert (got["mark"] == 0).all() and not got["front"].any() and got["nelem"].tolist() == [6000]


@pytest.mark.gpu
def test_a_thousand_colours(ctx):
    """many colours in every block's table (a few hundred keys in 1024 slots; no key is pushed out: that is
    test_a_block_table_overflows): the counts per previous colour stay exact"""
    g = R.mesh_case("a", True)
    mark = np.random.default_rng(8).integers(0, 1000, 6000).astype(np.int32)
    w = (np.random.default_rng(9).permutation(1000) + 1).astype(np.int32)
    nelem = np.full(1000, 1 << 20, np.int32)  # local and never short: nelem records D
    want = M.ifc_seq(g["tetv"], g["adja"], mark, w, nelem, M.nemin_of(nelem), g["np"], 1)
    got = layers(ctx, g["tetv"], g["np"], mark, w, nelem, M.nemin_of(nelem), 1)
    assert_state(got, want[0])
    assert (nelem - got["nelem"]).sum() >= got["moved"][0] > 1000


def remap(ctx, tetv, mark, ncolor, order, layout="tetv"):
    dt, d8 = mesh_args(ctx, tetv, layout)
    (dm,) = up(ctx, np.asarray(mark, np.int32))
    pb, part = guarded(ctx, np.full(len(mark), SENT))
    n = ctypes.c_int(-1)
    ok = ctx.lib.pmmg_hip_remap_colors(ctx.h, len(tetv), P(dt), P(d8), P(dm), ncolor,
                                       np.ascontiguousarray(order, np.int32).ctypes.data_as(ctypes.c_void_p), P(part),
                                       ctypes.byref(n))
    out = unguard(pb, len(mark))
    free(dt, d8, dm)
    assert ok == 1, ctx.error()
    return out, n.value


@pytest.mark.gpu
@pytest.mark.parametrize("layout", ["tetv", "tet8"])
def test_remap_colors(ctx, layout):
    g = R.mesh_case("b", True)
    mark = (2 * g["part"] + 1).astype(np.int32)  # 8 of 20 colours present
    order = np.roll(np.arange(20), 7).astype(np.int32)
    part, ngrp = remap(ctx, g["tetv"], mark, 20, order, layout)
    want, n = M.remap(g["tetv"], mark, 20, order)
    np.testing.assert_array_equal(part, want)
    assert ngrp == n == 8 and sorted(set(part.tolist())) == list(range(8))


@functools.lru_cache(maxsize=None)
def big():
    bg = synth.lattice(synth.CUBE, 56, jitter=0.1, seed=5)
    x = bg.xyz[bg.tetv - 1, 0].mean(axis=1)
    x = (x - x.min()) / (x.max() - x.min())
    return bg, np.minimum((x * 8).astype(np.int32), 7)


@pytest.mark.gpu
def test_a_million_tetra_against_the_definition(ctx):
    """the second trip of the grid-stride loops (more than 2048 blocks of 256)"""
    bg, mark = big()
    assert bg.ne > 2048 * 256 * 2
    w = np.array([4, 8, 2, 6, 1, 7, 3, 5], np.int32)
    none = np.full(8, -1, np.int32)
    want = M.ifc_par(bg.tetv, mark, w, none, none * 0, bg.np, 2)
    dev = (ctx.upload(np.ascontiguousarray(bg.tetv)), None)
    try:
        got = layers(ctx, bg.tetv, bg.np, mark, w, none, none * 0, 2, dev=dev)
    finally:
        free(dev[0])
    assert_state(got, want["layers"][1])
    assert got["moved"].tolist() == [l["moved"] for l in want["layers"]] and got["moved"].min() > 0


# the launch shape of k_ifc_sweep (pmmg_moveifc.hip): blocks of 256, at most 2048 of them, a table of 1024 slots
# per block hashed by (colour * 2654435761 mod 2^32) >> 22, 8 slots tried before the global word is used
K_BLOCK, K_MAXBLOCKS, K_SLOTS, K_PROBE = 256, 2048, 1024, 8


def table_home(colour):
    return ((np.asarray(colour, np.uint64) * np.uint64(2654435761)) & np.uint64(0xFFFFFFFF)) >> np.uint64(22)


@pytest.mark.gpu
def test_a_block_table_overflows(ctx):
    """the route past a block's table, to the global word: on the million-tetra lattice every mark is drawn from
    the 3000 lowest colours of 65536 whose slot lies below 48.  A key is placed at most 7 slots after its own,
    so a block's keys fit in 55 slots whatever order they arrive in; every block re-marks tetra of hundreds of
    different colours (shown on the host from the definition's result): all but 55 of them go to the global word.
    The counts per previous colour, read off nelem, stay exact."""
    bg, _ = big()
    ncolor = 1 << 16
    home = table_home(np.arange(ncolor))
    pool = np.nonzero(home < 48)[0][:3000].astype(np.int32)
    assert pool.size == 3000
    mark = pool[np.random.default_rng(12).integers(0, 3000, bg.ne)]
    w = (np.random.default_rng(13).permutation(ncolor) + 1).astype(np.int32)
    nelem = np.full(ncolor, 1 << 20, np.int32)  # local and never short: nelem records D
    nemin = M.nemin_of(nelem)
    want = M.ifc_par(bg.tetv, mark, w, nelem, nemin, bg.np, 1)
    assert want["blocked"] == 0
    # on the host: the first event of a re-marked tetra has the tetra's old mark as its previous colour
    grid = min(K_MAXBLOCKS, -(-bg.ne // K_BLOCK))
    block = (np.arange(bg.ne) // K_BLOCK) % grid
    moved = want["layers"][0]["mark"] != mark
    keys = np.unique(block[moved].astype(np.int64) * ncolor + mark[moved])
    per_block = np.bincount(keys // ncolor, minlength=grid)
    print("distinct previous colours per block:", per_block.min(), "to", per_block.max(), "in", 48 + K_PROBE - 1, "slots")
    assert (table_home(mark) < 48).all() and per_block.min() > 48 + K_PROBE - 1
    dev = (ctx.upload(np.ascontiguousarray(bg.tetv)), None)
    try:
        got = layers(ctx, bg.tetv, bg.np, mark, w, nelem, nemin, 1, dev=dev)
    finally:
        free(dev[0])
    assert_state(got, want["layers"][0])
    assert got["moved"].tolist() == [want["layers"][0]["moved"]]
    assert (nelem - got["nelem"]).sum() >= got["moved"][0] > bg.ne // 2


# ---------------------------------------------------------------- 3. the brake

@pytest.mark.gpu
def test_brake_at_the_threshold_and_one_past_it(ctx):
    (tetv, adja, mark, w, np_), d1 = brake_fixture()
    free_run = M.ifc_par(tetv, mark, w, np.array([-1, -1]), np.array([0, 0]), np_, 2)
    l1 = free_run["layers"][0]
    d2 = int(M.layer_par(tetv, l1["mark"], w, np.array([-1, -1]), np.array([0, 0]), l1["color"], l1["front"])["D"][1])
    assert d1 > 0 and d2 > 0
    nemin = np.array([6, 6], np.int32)
    at = np.array([40, d1 + d2 + 6], np.int32)  # D == negrp - nemin in the second layer
    want = M.ifc_seq(tetv, adja, mark, w, at, nemin, np_, 2)
    got = layers(ctx, tetv, np_, mark, w, at, nemin, 2)
    assert (got["done"], got["blocked"]) == (2, 0) and got["nelem"].tolist() == [40, 6]
    assert_state(got, want[1])
    past = np.array([40, d1 + d2 + 5], np.int32)
    want = M.ifc_seq(tetv, adja, mark, w, past, nemin, np_, 2)
    assert want[0]["abandoned"] == 0 and want[1]["abandoned"] >= 1
    got = layers(ctx, tetv, np_, mark, w, past, nemin, 2)
    assert (got["done"], got["blocked"]) == (1, 1)
    assert_state(got, want[0], "the layer before the blocked one")
    assert got["nelem"].tolist() == [40, d2 + 5] and got["moved"].tolist() == [want[0]["moved"], 0]
    # blocked in the first layer: nothing at all is written
    first = np.array([40, d1 + 5], np.int32)
    s = seed(ctx, tetv, np_, mark, w)
    got = layers(ctx, tetv, np_, mark, w, first, nemin, 2)
    assert (got["done"], got["blocked"]) == (0, 1) and got["nelem"].tolist() == first.tolist()
    np.testing.assert_array_equal(got["mark"], mark)
    np.testing.assert_array_equal(got["color"], s["color"])
    np.testing.assert_array_equal(got["front"], s["front"])


@pytest.mark.gpu
def test_a_blocked_layer_drops_its_set_points(ctx):
    """set points given, the second layer blocked: the outputs are the loop's after the first layer, without the
    front flags the second layer's set points had been given"""
    (tetv, adja, mark, w, np_), _ = brake_fixture()
    sp, sc = np.array([6, 16, 27], np.int32), np.array([0, 0, 0], np.int32)
    nemin = np.array([6, 6], np.int32)
    big_n = np.array([1 << 20, 1 << 20], np.int32)
    free_run = M.ifc_par(tetv, mark, w, big_n, nemin, np_, 2, sp, sc)
    d1 = int(big_n[1] - free_run["layers"][0]["nelem"][1])
    d2 = int(free_run["layers"][0]["nelem"][1] - free_run["layers"][1]["nelem"][1])
    assert d1 > 0 and d2 > 0
    past = np.array([1 << 20, d1 + d2 + 5], np.int32)
    want = M.ifc_seq(tetv, adja, mark, w, past, nemin, np_, 2, sp, sc)
    assert want[0]["abandoned"] == 0 and want[1]["abandoned"] >= 1
    assert not want[0]["front"][sp - 1].all()  # (a set point that nothing touched left the front again)
    got = layers(ctx, tetv, np_, mark, w, past, nemin, 2, set_pt=sp, set_color=sc)
    assert (got["done"], got["blocked"]) == (1, 1)
    assert_state(got, want[0], "the layer before the blocked one")
    at = np.array([1 << 20, d1 + d2 + 6], np.int32)
    got = layers(ctx, tetv, np_, mark, w, at, nemin, 2, set_pt=sp, set_color=sc)
    assert (got["done"], got["blocked"]) == (2, 0)
    assert_state(got, M.ifc_seq(tetv, adja, mark, w, at, nemin, np_, 2, sp, sc)[1])


# ---------------------------------------------------------------- 4. refusals, determinism, side effects

@pytest.mark.gpu
def test_refusals_leave_everything_untouched(ctx):
    tetv, _, np_ = M.path_mesh(65)
    mark, w = M.bands(65, 5, 3), np.array([3, 1, 2], np.int32)
    none = np.full(3, -1, np.int32)
    good = seed(ctx, tetv, np_, mark, w)
    badmark, badvert = mark.copy(), tetv.copy()
    badmark[40] = 3
    badvert[64, 2] = np_ + 1
    cases = [
        ("a mark", dict(mark=badmark)), ("not positive", dict(w=np.array([3, 0, 2], np.int32))),
        ("a vertex id", dict(tetv=badvert)), ("exceed", dict(ne=1 << 29)),
    ]
    for text, kw in cases:
        a = dict(tetv=tetv, mark=mark, w=w)
        a.update({k: v for k, v in kw.items() if k != "ne"})
        s = seed(ctx, a["tetv"], np_, a["mark"], a["w"], ne=kw.get("ne"), want_ok=False)
        assert s["ok"] == 0 and text in s["msg"], s["msg"]
        assert (s["color"] == SENT).all() and (s["front"] == 0x77).all()
        got = layers(ctx, a["tetv"], np_, a["mark"], a["w"], none, none * 0, 2, color=good["color"],
                     front=good["front"], ne=kw.get("ne"), want_ok=False)
        assert got["ok"] == 0 and text in got["msg"], got["msg"]
        np.testing.assert_array_equal(got["mark"], a["mark"])
        np.testing.assert_array_equal(got["color"], good["color"])
        np.testing.assert_array_equal(got["front"], good["front"])
        assert (got["moved"] == SENT).all() and (got["done"], got["blocked"]) == (SENT, SENT)
    for text, kw in [("set_pt", dict(set_pt=[5, np_ + 1])), ("set_pt", dict(set_pt=[0])),
                     ("set_color", dict(set_pt=[5], set_color=[3]))]:
        got = layers(ctx, tetv, np_, mark, w, none, none * 0, 2, color=good["color"], front=good["front"],
                     want_ok=False, **kw)
        assert got["ok"] == 0 and text in got["msg"], got["msg"]
        np.testing.assert_array_equal(got["mark"], mark)
        np.testing.assert_array_equal(got["color"], good["color"])
        assert (got["moved"] == SENT).all() and (got["done"], got["blocked"]) == (SENT, SENT)
    # a point colour outside the colours, at a point of a used tetra
    bad = good["color"].copy()
    bad[10] = -1
    got = layers(ctx, tetv, np_, mark, w, none, none * 0, 1, color=bad, front=good["front"], want_ok=False)
    assert got["ok"] == 0 and "colour of a point" in got["msg"] and (got["moved"] == SENT).all()
    # alignment: tetv 16 bytes
    raw = ctx.upload(np.zeros(4 * 65 + 4, np.int32))
    off = DeviceArray(raw.ptr + 4, 16 * 65, (65, 4), np.dtype(np.int32), ctx)
    (dm,) = up(ctx, mark)
    cb, color = guarded(ctx, np.full(np_, SENT))
    fb, front = guarded_bytes(ctx, np.full(np_, 0x77))
    ok = ctx.lib.pmmg_hip_ifc_seed(ctx.h, np_, 65, P(off), None, P(dm), 3, w.ctypes.data_as(ctypes.c_void_p), P(color),
                                   P(front))
    assert ok == 0 and "aligned" in ctx.error()
    assert (unguard(cb, np_) == SENT).all() and (unguard_bytes(fb, np_) == 0x77).all()
    free(raw, dm)


def shifted(ctx, values, by):
    """(buffer, an int32 device array `by` bytes past a 256-byte guard, filled with values)"""
    values = np.ascontiguousarray(values, np.int32)
    raw = np.full(2 * GUARD + 4 * values.size + 16, FILL, np.uint8)
    raw[GUARD + by:GUARD + by + 4 * values.size] = values.view(np.uint8).reshape(-1)
    buf = ctx.upload(raw)
    return buf, DeviceArray(buf.ptr + GUARD + by, 4 * values.size, values.shape, np.dtype(np.int32), ctx), raw


@pytest.mark.gpu
def test_alignment_and_remap_refusals(ctx):
    """tetv 16 bytes, every other int array 4 bytes, in all three calls; a mark outside the colours in
    remap_colors: 0, a message, and not a byte of an output or of *ngrp changed"""
    tetv, _, np_ = M.path_mesh(65)
    mark, w = M.bands(65, 5, 3), np.array([3, 1, 2], np.int32)
    order = np.arange(3, dtype=np.int32)
    good = seed(ctx, tetv, np_, mark, w)
    vp = lambda a: a.ctypes.data_as(ctypes.c_void_p)
    none = np.full(3, -1, np.int32)
    for what in ("tetv", "mark", "ptcolor", "set_pt", "part"):
        tb, dt, _ = shifted(ctx, tetv, 4 if what == "tetv" else 0)
        mb, dm, mraw = shifted(ctx, mark, 2 if what == "mark" else 0)
        cb, dc, craw = shifted(ctx, good["color"], 2 if what == "ptcolor" else 0)
        sb, dsp, _ = shifted(ctx, np.array([5], np.int32), 2 if what == "set_pt" else 0)
        pb, dpart, praw = shifted(ctx, np.full(65, SENT), 2 if what == "part" else 0)
        fb, dfront = guarded_bytes(ctx, good["front"])
        done, blocked, ngrp = ctypes.c_int(SENT), ctypes.c_int(SENT), ctypes.c_int(SENT)
        moved, nelem = np.full(1, SENT, np.int32), none.copy()
        calls = []
        if what in ("tetv", "mark", "ptcolor"):
            calls.append(("ifc_seed", lambda: ctx.lib.pmmg_hip_ifc_seed(ctx.h, np_, 65, P(dt), None, P(dm), 3, vp(w), P(dc),
                                                                        P(dfront))))
        if what != "part":
            calls.append(("ifc_layers", lambda: ctx.lib.pmmg_hip_ifc_layers(
                ctx.h, np_, 65, P(dt), None, P(dm), 3, vp(w), vp(nelem), vp(none * 0), P(dc), P(dfront), 1, P(dsp), None, 1,
                ctypes.byref(done), ctypes.byref(blocked), vp(moved))))
        if what in ("tetv", "mark", "part"):
            calls.append(("remap_colors", lambda: ctx.lib.pmmg_hip_remap_colors(ctx.h, 65, P(dt), None, P(dm), 3, vp(order),
                                                                                P(dpart), ctypes.byref(ngrp))))
        for name, call in calls:
            assert call() == 0 and "aligned" in ctx.error() and name in ctx.error(), (what, name, ctx.error())
        assert (done.value, blocked.value, ngrp.value, moved[0]) == (SENT,) * 4 and (nelem == -1).all()
        for buf, raw in ((mb, mraw), (cb, craw), (pb, praw)):
            assert buf.download().tobytes() == raw.tobytes(), what
        np.testing.assert_array_equal(unguard_bytes(fb, np_), good["front"])
        free(tb, mb, cb, sb, pb)
    # remap_colors: a mark of a used tetra outside the colours
    bad = mark.copy()
    bad[40] = 3
    dt, dm = up(ctx, tetv, bad)
    pb, part = guarded(ctx, np.full(65, SENT))
    ngrp = ctypes.c_int(SENT)
    assert ctx.lib.pmmg_hip_remap_colors(ctx.h, 65, P(dt), None, P(dm), 3, vp(order), P(part), ctypes.byref(ngrp)) == 0
    assert "a mark" in ctx.error() and ngrp.value == SENT and (unguard(pb, 65) == SENT).all()
    free(dt, dm)


@pytest.mark.gpu
def test_two_calls_and_release_scratch(ctx):
    g, w, nelem, nemin = case_inputs(("b", True), "ties", True)
    runs = []
    for i in range(3):
        if i == 2:
            ctx.release_scratch()
        runs.append(layers(ctx, g["tetv"], g["np"], g["part"], w, nelem, nemin, 2))
    for key in ("mark", "color", "front", "nelem", "moved"):
        assert runs[0][key].tobytes() == runs[1][key].tobytes() == runs[2][key].tobytes(), key


@pytest.mark.gpu
def test_transfer_does_not_see_the_moveifc_scratch():
    g, w, nelem, nemin = case_inputs(("b", False), "perm", False)
    case = make_case(kind=synth.CUBE, n_old=6, n_new=7, with_ref=False)
    with TransferContext(0) as c:
        before = run_gpu(case, ctx=c)
        got = layers(c, g["tetv"], g["np"], g["part"], w, nelem, nemin, 2)
        assert_state(got, seq(("b", False), "perm", False, False)[1])
        after = run_gpu(case, ctx=c)
    same_outputs(before, run_gpu(case))
    same_outputs(before, after)


# ---------------------------------------------------------------- 5. the chain and the upper layers

def _outputs(groups):
    return [dict(met=g["met_out"].download(), fields=[f.download() for f in g["fields_out"]],
                 elem=g["elem_out"].download(), hit=g["hit_out"].download()) for g in groups]


@pytest.mark.gpu
def test_move_then_split_then_transfer(ctx):
    """marks -> moved marks -> fix -> packed colours -> split -> transfer of the groups, all on the device: the moved
    marks are those of the restatements, every colour is one subgroup after the fix, and the transfer against the
    groups is bit-identical to the same transfer on groups cut on the host from the same partition"""
    import split_ref as S

    case = make_case(kind=synth.CUBE, n_old=6, n_new=7, with_ref=False)
    bg, new = case["bg"], case["new"]
    slab = lambda x: np.minimum((x * 2).astype(np.int32), 1)  # two slabs, three cells wide: a layer takes one
    mark = slab(bg.xyz[bg.tetv - 1, 0].mean(axis=1))
    nelem = np.bincount(mark, minlength=2).astype(np.int32)
    w = nelem + np.array([1, 0], np.int32)  # the upper slab wins; its tetra come second, so the interface is front
    tetv, adja, dmark, dxyz, dmet = up(ctx, bg.tetv, bg.adja, mark, bg.xyz, case["met"])
    dfields = up(ctx, *case["fields"])
    color, front = ctx.interface_points(bg.np, dmark, w, tetv=tetv)
    res = ctx.move_interfaces(bg.np, dmark, w, nelem, tetv=tetv, adja=adja, ptcolor=color, ptfront=front, nlayers=2)
    assert (res["layers_done"], res["blocked"]) == (2, 0) and res["moved"].min() > 0
    want = M.ifc_seq(bg.tetv, bg.adja, mark, w, nelem, M.nemin_of(nelem), bg.np, 2)[1]
    fixed = R.fix_free(bg.adja, want["mark"], 2)
    np.testing.assert_array_equal(dmark.download(), fixed["part"])
    np.testing.assert_array_equal(res["nelem"], want["nelem"])
    assert res["fix"]["nmoved"] == fixed["nmoved"]
    sub = ctx.part_subgroups(tetv, adja=adja, part=dmark, ncolor=2)
    assert sub["ncomp"].tolist() == [1, 1]
    dpart, ngrp = ctx.remap_colors(dmark, 2, tetv=tetv)
    assert ngrp == 2
    part = dpart.download()
    np.testing.assert_array_equal(part, fixed["part"])
    assert (part != mark).sum() > 0
    sp = ctx.split_groups(bg.np, dpart, ngrp, tetv=tetv, adja=adja)
    dev_groups, owned = ctx.groups_from_split(sp, dxyz, dmet, dfields)
    cutw = S.split_seq(bg.tetv, bg.adja, part, 2, bg.np)
    te, pt, _, _ = S.segments(cutw)
    host_groups = []
    for g in range(2):
        tv, ad = cutw["tetv_out"][te[g]:te[g + 1]], cutw["adja_out"][te[g]:te[g + 1]]
        old = cutw["old_pt"][pt[g]:pt[g + 1]] - 1
        host_groups.append(dict(np=old.size, ne=tv.shape[0], xyz=ctx.upload(bg.xyz[old]),
                                tet8=ctx.upload(pack_tet8(tv, ad)), met=ctx.upload(case["met"][old]),
                                fields=[ctx.upload(f[old]) for f in case["fields"]]))
    # a new point goes to the group of the old tetra nearest to it along x (any assignment serves the comparison)
    qslab = slab(new.xyz[:, 0])
    keep = []
    for groups in (dev_groups, host_groups):
        for g, grp in enumerate(groups):
            q = np.ascontiguousarray(new.xyz[qslab == g])
            triv, adjt = ctx.build_boundary(grp["np"], tet8=grp["tet8"])
            grp.update(triv=triv, adjt=adjt, hausd=case["hausd"], xyz_new=ctx.upload(q),
                       pclass=ctx.upload(np.ascontiguousarray(case["pclass"][qslab == g])),
                       met_out=ctx.upload(np.full((q.shape[0], 6), np.nan)),
                       fields_out=[ctx.upload(np.full((q.shape[0], f.shape[1]), np.nan)) for f in case["fields"]],
                       elem_out=ctx.upload(np.zeros(q.shape[0], np.int32)), hit_out=ctx.upload(np.zeros(q.shape[0], np.int8)))
            keep += [triv, adjt, grp["xyz_new"], grp["pclass"], grp["met_out"], grp["elem_out"], grp["hit_out"]]
            keep += grp["fields_out"]
        ctx.locate_interp_groups(groups)
    for a, b in zip(_outputs(dev_groups), _outputs(host_groups)):
        same_outputs(a, b)
        assert (a["hit"] != 0).sum() > 0
    for grp in host_groups:
        keep += [grp["xyz"], grp["tet8"], grp["met"]] + grp["fields"]
    lists = ("old_pt", "face_idx1", "face_idx2", "node_idx1", "node_idx2")
    free(tetv, adja, dmark, dxyz, dmet, dpart, color, front, *dfields, *owned, *keep,
         *[sp[k] for k in ("old_tet", "new_tet", "tet8_out") + lists])


@pytest.mark.gpu
def test_host_layer_equals_the_device_path(ctx):
    # the first fixture whose two layers no brake stops with every colour local (by the definition, on the host)
    for case, wkind in [(c, k) for c in R.MESH_CASES for k in M.WEIGHTS]:
        g, w, nelem, nemin = case_inputs(case, wkind, True)
        if not M.ifc_par(g["tetv"], g["part"], w, nelem, nemin, g["np"], 2)["blocked"]:
            break
    else:
        raise AssertionError("no fixture runs two layers with every colour local")
    print("host layer on", case, wkind)
    tetv, adja, dmark = up(ctx, g["tetv"], g["adja"], g["part"])
    res = ctx.move_interfaces(g["np"], dmark, w, nelem, tetv=tetv, adja=adja, nlayers=2)
    want = dmark.download()
    free(tetv, adja, dmark, res["ptcolor"], res["ptfront"])
    lib = _native.host_lib()
    vp = lambda a: np.ascontiguousarray(a).ctypes.data_as(ctypes.c_void_p)
    out = np.full(6000, SENT, np.int32)
    done, blocked = ctypes.c_int(-1), ctypes.c_int(-1)
    tv, ad, mk = (np.ascontiguousarray(g[k]) for k in ("tetv", "adja", "part"))
    ok = lib.pmmg_part_move_interfaces(ctx.h, g["np"], 6000, vp(tv), vp(ad), vp(mk), g["ncolor"], vp(w), vp(nelem), 2,
                                       vp(out), ctypes.byref(done), ctypes.byref(blocked))
    assert ok == 1, ctx.error()
    assert (done.value, blocked.value) == (res["layers_done"], res["blocked"]) == (2, 0)
    np.testing.assert_array_equal(out, want)
    assert (out != g["part"]).sum() > 0
    bad = np.array(w)
    bad[1] = 0
    out[:] = SENT
    assert lib.pmmg_part_move_interfaces(ctx.h, g["np"], 6000, vp(tv), vp(ad), vp(mk), g["ncolor"], vp(bad), vp(nelem), 2,
                                         vp(out), None, None) == 0
    assert (out == SENT).all()
