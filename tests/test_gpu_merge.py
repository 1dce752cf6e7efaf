"""pmmg_hip_merge_groups and pmmg_hip_gather_rows_i32 against the restatements
of tests/merge_ref.py, exactly (runs on the MI355X).

tests/test_merge_ref_host.py shows, on the CPU, that merge_par (array
operations) equals merge_seq (the reference's loop, transcribed) on the
fixtures; here every output of the device is compared with merge_seq, and the
1M-tetra case, where the transcribed loop would take minutes, with merge_par.

Every call goes through merge(), which puts 256 guard bytes around every
device output and guard words around the host outputs, pre-fills the outputs
with SENT and checks that nothing beyond the merged points was written."""
import ctypes
import functools
import types

import numpy as np
import pytest

import contig_ref as R
import merge_ref as M
import snapshot_ref
import split_ref as S
from oracle import oracle as O
from parity import check, device_view, make_case, run_gpu, same_outputs
from parmmg_amd import _native, synth
from parmmg_amd.transfer import DeviceArray, TransferContext, pack_tet8
from test_gpu_contig import P, SENT, free, guarded, host_guarded, host_unguard, unguard, up
from test_merge_ref_host import HAND
from test_metis_graph import cut, fixture

OUTS = ("new_pt", "new_tet", "src_pt", "src_tet", "tetv_out", "mark_out", "node_val", "face_val")
LISTS = ("old_pt", "face_idx1", "face_idx2", "node_idx1", "node_idx2")


@pytest.fixture(scope="module")
def ctx():
    with TransferContext(0) as c:
        yield c


def merge(ctx, sp, color=None, tet8=False, pt_cap=None, outs=OUTS, nnode=None, nface=None, shift_tetv=0):
    """the C call on a split in split_ref's layout (host arrays), with guarded outputs.  pt_cap None: the groups'
    points.  Returns dict(ok, msg, np, ne, and every output as an array of its allocated length)."""
    count = np.ascontiguousarray(sp["count"], np.int32).reshape(-1, 4)
    ngrp = count.shape[0]
    nnode = int(sp["nnode_end"] if nnode is None else nnode)
    nface = int(sp["nface_end"] if nface is None else nface)
    tv = np.ascontiguousarray(sp["tetv_out"], np.int32).reshape(-1, 4)
    T, Pn = tv.shape[0], int(count[:, 1].sum())  # (the rows there are: a refusal case overstates the counts)
    cap = Pn if pt_cap is None else pt_cap
    rows = pack_tet8(tv, sp.get("adja_out", np.zeros_like(tv))) if tet8 else tv
    d_rows, rows_alloc = device_view(ctx, rows, shift_tetv)
    lists = up(ctx, *[np.ascontiguousarray(sp[k], np.int32) for k in ("node_idx1", "node_idx2", "face_idx1", "face_idx2")])
    lens = dict(new_pt=Pn, new_tet=T, src_pt=cap, src_tet=T, tetv_out=4 * T, mark_out=T, node_val=nnode, face_val=nface)
    if color is None:
        outs = tuple(k for k in outs if k != "mark_out")
    bufs = {k: guarded(ctx, np.full(lens[k], SENT)) for k in outs}
    d = lambda k: P(bufs[k][1]) if k in bufs else None
    cnt = (_native.HipSplitCount * ngrp)(*[_native.HipSplitCount(*[int(v) for v in r]) for r in count])
    col = None if color is None else np.ascontiguousarray(color, np.int32)
    ew, ep = host_guarded(2)
    try:
        ok = ctx.lib.pmmg_hip_merge_groups(
            ctx.h, ngrp, cnt, None if tet8 else P(d_rows), P(d_rows) if tet8 else None, *[P(a) for a in lists], nnode,
            nface, None if col is None else col.ctypes.data_as(ctypes.c_void_p), cap, d("new_pt"), d("new_tet"),
            d("src_pt"), d("src_tet"), d("tetv_out"), d("mark_out"), d("node_val"), d("face_val"),
            ctypes.cast(ep, ctypes.POINTER(ctypes.c_int)),
            ctypes.cast(ctypes.c_void_p(ep.value + 4), ctypes.POINTER(ctypes.c_int)))
        out = dict(ok=ok, msg=ctx.error())
        out["np"], out["ne"] = host_unguard(ew, 2).tolist()
        for k, (buf, view) in bufs.items():
            out[k] = unguard(buf, view.shape[0])
        rows_alloc.check("the tetra rows")
    finally:
        rows_alloc.free()
        free(*lists)
    return out


def assert_merge(got, want, outs=OUTS):
    """every output equal to the restatement's; nothing written beyond the merged points"""
    assert got["ok"] == 1, got["msg"]
    assert (got["np"], got["ne"]) == (want["np"], want["ne"])
    for k in outs:
        if k not in want or k not in got:
            assert k == "mark_out" or k not in got, k
            continue
        w = np.asarray(want[k], np.int32).reshape(-1)
        np.testing.assert_array_equal(got[k][:w.size], w, err_msg=k)
        assert (got[k][w.size:] == SENT).all(), k


def run_case(ctx, sp, color=None, ref=M.merge_seq, **kw):
    want = ref(sp, color=color, nnode=kw.get("nnode"), nface=kw.get("nface"))
    got = merge(ctx, sp, color=color, **kw)
    assert_merge(got, want)
    return got, want


def split_of(tetv, adja, part, ngrp, npv, **kw):
    return S.split_seq(np.ascontiguousarray(tetv, np.int32), np.ascontiguousarray(adja, np.int32),
                       np.ascontiguousarray(part, np.int32), ngrp, npv, **kw)


# ---------------------------------------------------------------- 1. structure

@pytest.mark.gpu
def test_one_group(ctx):
    """the identity, and the lists of group 0 as they stand in the two values arrays"""
    g = R.mesh_case("a", True)
    node_pos, face_old, nnode0, nface0 = S.old_positions(g["tetv"], g["adja"], 7)
    sp = split_of(g["tetv"], g["adja"], np.zeros(6000), 1, g["np"], node_pos=node_pos, face_old=face_old, nnode0=nnode0,
                  nface0=nface0)
    got, _ = run_case(ctx, sp, color=[5])
    np.testing.assert_array_equal(got["new_pt"], np.arange(1, g["np"] + 1))
    np.testing.assert_array_equal(got["src_tet"], np.arange(1, 6001))
    np.testing.assert_array_equal(got["tetv_out"], sp["tetv_out"].reshape(-1))
    assert (got["mark_out"] == 5).all() and (got["node_val"] > 0).sum() == nnode0 and (got["face_val"] > 0).sum() == nface0
    np.testing.assert_array_equal(got["face_val"][sp["face_idx2"]], sp["face_idx1"])


@pytest.mark.gpu
@pytest.mark.parametrize("which", sorted(HAND))
def test_hand_written(ctx, which):
    """the fixtures of tests/test_merge_ref_host.py against their hand-written arrays"""
    sp, color, want = HAND[which]()
    got = merge(ctx, sp, color=color)
    assert_merge(got, want)


@pytest.mark.gpu
@pytest.mark.parametrize("empty", ["first", "middle", "last", "all but one"])
def test_empty_groups(ctx, empty):
    g = R.mesh_case("b", False)
    part, nc = g["part"].astype(np.int32), g["ncolor"]
    if empty == "first":
        part, ngrp = part + 1, nc + 1
    elif empty == "middle":
        part, ngrp = np.where(part >= 1, part + 1, part).astype(np.int32), nc + 1
    elif empty == "last":
        ngrp = nc + 2
    else:
        part, ngrp = np.full(6000, 2, np.int32), 5
    sp = split_of(g["tetv"], g["adja"], part, ngrp, g["np"])
    assert (sp["count"][:, 0] == 0).any()
    got, _ = run_case(ctx, sp, color=100 + np.arange(ngrp))
    if sp["count"][0, 0] == 0:  # group 0 empty: every listed point is created, in order of its position's lowest entry
        listed = np.unique(sp["node_idx2"]).size
        assert got["np"] == g["np"] and (listed > 0) == (empty == "first")
        _, first = np.unique(sp["node_idx2"], return_index=True)
        te, pt, fa, no = S.segments(sp)
        grp = np.repeat(np.arange(ngrp), sp["count"][:, 3])
        rows = (pt[grp] + sp["node_idx1"])[np.sort(first)]
        np.testing.assert_array_equal(got["src_pt"][:listed], rows)


@pytest.mark.gpu
def test_every_tetra_a_group(ctx):
    """many holders per node (the most groups the position words see at one address): the sign's parity"""
    bg, _ = fixture()
    m = 320
    a = np.ascontiguousarray(cut(bg.adja, np.arange(bg.ne) < m)[:m])
    npv, tetv = snapshot_ref.prefix((bg.np, bg.tetv), m)
    part = np.random.default_rng(4).permutation(m).astype(np.int32)
    sp = split_of(tetv, a, part, m, npv)
    holders = np.bincount(sp["node_idx2"], minlength=sp["nnode_end"])
    assert holders.max() >= 8 and (holders % 2 == 0).any() and (holders[holders > 0] % 2 == 1).any()
    got, _ = run_case(ctx, sp, color=np.arange(m)[::-1])
    np.testing.assert_array_equal(got["node_val"] > 0, holders % 2 == 1)
    np.testing.assert_array_equal(got["node_val"] < 0, (holders > 0) & (holders % 2 == 0))
    assert got["np"] == npv


@pytest.mark.gpu
@pytest.mark.parametrize("m", [1, 63, 64, 65, 255, 256, 257, 2047, 2048, 2049, 4097])
def test_sizes(ctx, m):
    """the wave, block and scan-chunk edges: a prefix of the lattice in up to three groups of consecutive tetra,
    whose boundaries (m / 3, 2 m / 3) fall inside a wave, a block and a scan chunk"""
    bg, _ = fixture()
    npv, tetv = snapshot_ref.prefix((bg.np, bg.tetv), m)
    adja, non = snapshot_ref.adjacency(tetv)
    assert not non
    ngrp = min(3, m)
    part = (np.arange(m) * ngrp) // m
    assert all(int(b) % 64 for b in np.nonzero(np.diff(part))[0] + 1) or m < 64
    sp = split_of(tetv, adja, part, ngrp, npv)
    got, _ = run_case(ctx, sp, color=[3, 1, 2][:ngrp])
    assert got["np"] == npv and got["ne"] == m


@pytest.mark.gpu
def test_no_tetra(ctx):
    sp = dict(count=np.zeros((3, 4), np.int32), tetv_out=np.zeros((0, 4), np.int32), nnode_end=5, nface_end=2,
              **{k: np.zeros(0, np.int32) for k in LISTS[1:]})
    got, _ = run_case(ctx, sp, color=[1, 2, 3])
    assert (got["np"], got["ne"]) == (0, 0) and (got["node_val"] == 0).all() and (got["face_val"] == 0).all()


# ---------------------------------------------------------------- 2. the fixtures, on every layout

@functools.lru_cache(maxsize=None)
def mesh_reference(name, old):
    g = R.mesh_case(*name)
    kw = {}
    if old:
        node_pos, face_old, nnode0, nface0 = S.old_positions(g["tetv"], g["adja"], 7)
        kw = dict(node_pos=node_pos, face_old=face_old, nnode0=nnode0, nface0=nface0)
    sp = S.split_seq(g["tetv"], g["adja"], g["part"], g["ncolor"], g["np"], **kw)
    color = 10 + 3 * np.arange(g["ncolor"])
    return g, sp, color, M.merge_seq(sp, color=color)


@pytest.mark.gpu
@pytest.mark.parametrize("name", R.MESH_CASES, ids=str)
def test_mesh_fixtures(ctx, name):
    g, sp, color, want = mesh_reference(name, False)
    a = merge(ctx, sp, color=color)
    b = merge(ctx, sp, color=color, tet8=True)
    c = merge(ctx, sp, color=None, tet8=True, outs=("new_pt", "src_pt", "src_tet", "tetv_out"))
    assert_merge(a, want)
    for k in OUTS:
        assert a[k].tobytes() == b[k].tobytes(), k
        if k in c:
            assert a[k].tobytes() == c[k].tobytes(), k
    assert c["ok"] == 1 and "mark_out" not in c and "node_val" not in c
    _, sp_old, _, want_old = mesh_reference(name, True)
    d = merge(ctx, sp_old, color=color)
    assert_merge(d, want_old)
    for k in ("new_tet", "src_tet", "mark_out"):  # the old positions add entries of boundary faces: not the tetra's places
        assert d[k].size == a[k].size
    # the round trip, from the device's maps alone
    tet, pnt = sp["old_tet"][a["src_tet"] - 1], sp["old_pt"][a["src_pt"][:a["np"]] - 1]
    assert sorted(tet.tolist()) == list(range(1, 6001)) and sorted(pnt.tolist()) == list(range(1, g["np"] + 1))
    np.testing.assert_array_equal(pnt[a["tetv_out"].reshape(-1, 4) - 1], g["tetv"][tet - 1])


# ---------------------------------------------------------------- 3. the second trip of every grid-stride loop

def slabs_and_islands(mesh, nslab, nisland, seed):
    u = mesh.xyz[mesh.tetv - 1].mean(axis=1)
    u = (u - u.min(axis=0)) / np.ptp(u, axis=0)
    part = np.minimum((u[:, 0] * nslab).astype(np.int32), nslab - 1)
    return R._islands(u, part, nslab, nisland, np.random.default_rng(seed)).astype(np.int32)


@functools.lru_cache(maxsize=None)
def big(numbering):
    mesh = synth.lattice(synth.CUBE, 56, with_trias=False)
    part = slabs_and_islands(mesh, 16, 30, 9)
    tetv, adja = mesh.tetv, mesh.adja
    if numbering == "mmg":
        perm = synth.mmg_like_perm(mesh.ne)
        tetv, adja = R.permuted(tetv, adja, perm)
        part = np.ascontiguousarray(part[perm])
    assert mesh.ne == 6 * 56 ** 3 > 2048 * 256  # more tetra than the grid-stride kernels have threads
    return tetv, adja, part, int(mesh.np)


def download_split(sp):
    out = {k: sp[k].download() for k in ("old_tet", "tetv_out") + LISTS}
    out.update(count=sp["count"], nnode_end=sp["nnode_end"], nface_end=sp["nface_end"])
    return out


@pytest.mark.gpu
@pytest.mark.parametrize("numbering", ["lattice", "mmg"])
def test_one_million_tetra(ctx, numbering):
    """the groups come from the device's split (held against split_par by tests/test_gpu_split.py); the merge of
    the downloaded groups by merge_par is what the device's merge must give, and the round trip closes"""
    tetv, adja, part, npv = big(numbering)
    dev = up(ctx, tetv, adja, part)
    sp = ctx.split_groups(npv, dev[2], 16, tetv=dev[0], adja=dev[1], want=("tetv_out",))
    color = np.arange(16, dtype=np.int32) * 7
    mg = ctx.merge_groups(sp, color=color)
    try:
        host = download_split(sp)
        want = M.merge_par(host, color=color)
        assert (mg["np"], mg["ne"]) == (want["np"], want["ne"]) == (npv, tetv.shape[0])
        for k in OUTS:
            np.testing.assert_array_equal(mg[k].download().reshape(-1), want[k].reshape(-1), err_msg=k)
        tet, pnt = host["old_tet"][want["src_tet"] - 1], host["old_pt"][want["src_pt"] - 1]
        np.testing.assert_array_equal(pnt[want["tetv_out"] - 1], tetv[tet - 1])
        assert (want["node_val"] < 0).sum() > 0 and (want["face_val"] < 0).sum() == sp["nface_end"]
    finally:
        free(*dev, *[sp[k] for k in ("old_tet", "tetv_out") + LISTS], *[mg[k] for k in OUTS])


# ---------------------------------------------------------------- 4. caps, refusals

@pytest.mark.gpu
def test_caps(ctx):
    g, sp, color, want = mesh_reference(("b", True), False)
    for cap in (0, want["np"] - 1):
        got = merge(ctx, sp, color=color, pt_cap=cap)
        assert got["ok"] == 0 and "pt_cap" in got["msg"], got["msg"]
        assert (got["np"], got["ne"]) == (want["np"], want["ne"])
        for k in OUTS:
            assert (got[k] == SENT).all(), k
    assert_merge(merge(ctx, sp, color=color, pt_cap=want["np"]), want)
    assert_merge(merge(ctx, sp, color=color, pt_cap=want["np"] + 5), want)


REFUSALS = ["vertex 0", "vertex np+1", "node index1 0", "node index1 np+1", "node index2 -1", "node index2 nnode",
            "face index1 11", "face index1 12(ne+1)", "face index2 -1", "face index2 nface", "tetra limit",
            "misaligned tetv", "negative count"]


@pytest.mark.gpu
@pytest.mark.parametrize("what", REFUSALS)
def test_refusals(ctx, what):
    """each returns 0 with its message and every output still the fill value, inside and around the arrays"""
    g, sp0, color, _ = mesh_reference(("a", False), False)
    sp = {k: (np.array(v) if isinstance(v, np.ndarray) else v) for k, v in sp0.items()}
    te, pt, fa, no = S.segments(sp)
    grp = 1
    np_g, ne_g = int(sp["count"][grp, 1]), int(sp["count"][grp, 0])
    kw, word = {}, what.split()[0]
    if what.startswith("vertex"):
        sp["tetv_out"][te[grp] + 7, 2] = 0 if what == "vertex 0" else np_g + 1
    elif what.startswith("node index1"):
        sp["node_idx1"][no[grp] + 3], word = (0 if what.endswith(" 0") else np_g + 1), "node index1"
    elif what.startswith("node index2"):
        sp["node_idx2"][no[2] - 1], word = (-1 if what.endswith("-1") else sp["nnode_end"]), "node index2"
    elif what.startswith("face index1"):
        sp["face_idx1"][fa[grp] + 5], word = (11 if what.endswith("11") else 12 * (ne_g + 1)), "face index1"
    elif what.startswith("face index2"):
        sp["face_idx2"][fa[grp]], word = (-1 if what.endswith("-1") else sp["nface_end"]), "face index2"
    elif what == "tetra limit":
        sp["count"] = sp["count"].copy()
        sp["count"][2, 0] += 178956970 - 6000
        word = "12*ie+11"
    elif what == "misaligned tetv":
        kw, word = dict(shift_tetv=4), "16-byte"
    else:
        sp["count"] = sp["count"].copy()
        sp["count"][1, 3] = -1
        word = "negative"
    got = merge(ctx, sp, color=color, **kw)
    assert got["ok"] == 0 and word in got["msg"], got["msg"]
    for k in OUTS:
        assert (got[k] == SENT).all(), k


# ---------------------------------------------------------------- 5. determinism, isolation

@pytest.mark.gpu
def test_two_calls_and_release_scratch(ctx):
    g, sp, color, want = mesh_reference(("c", True), True)
    a = merge(ctx, sp, color=color)
    b = merge(ctx, sp, color=color)
    ctx.release_scratch()
    c = merge(ctx, sp, color=color)
    assert_merge(a, want)
    for k in OUTS:
        assert a[k].tobytes() == b[k].tobytes() == c[k].tobytes(), k


@pytest.mark.gpu
def test_transfer_does_not_see_the_merge_scratch():
    g, sp, color, want = mesh_reference(("b", False), False)
    case = make_case(kind=synth.CUBE, n_old=6, n_new=7, with_ref=False)
    with TransferContext(0) as c:
        before = run_gpu(case, ctx=c)
        assert_merge(merge(c, sp, color=color), want)
        after = run_gpu(case, ctx=c)
    same_outputs(before, run_gpu(case))
    same_outputs(before, after)


# ---------------------------------------------------------------- 6. gather_rows_i32

@pytest.mark.gpu
@pytest.mark.parametrize("size", [1, 3, 4])
@pytest.mark.parametrize("offset", [0, 4, 8])
def test_gather_rows_i32(ctx, size, offset):
    rng = np.random.default_rng(size)
    rows = rng.integers(-2 ** 31, 2 ** 31 - 1, (500, size)).astype(np.int32)
    d_rows, rows_alloc = device_view(ctx, rows, offset)
    try:
        for n in (0, 1, 63, 64, 65, 4097):
            src = rng.integers(1, 501, n).astype(np.int32)  # (with repeats)
            d_src, src_alloc = device_view(ctx, src, 4)
            d_out, out_alloc = device_view(ctx, np.full((n, size), SENT, np.int32), offset)
            ok = ctx.lib.pmmg_hip_gather_rows_i32(ctx.h, n, P(d_src), size, P(d_rows), P(d_out))
            assert ok == 1, ctx.error()
            np.testing.assert_array_equal(d_out.download(), rows[src - 1])
            for al in (src_alloc, out_alloc):
                al.check("gather_rows_i32 n=%d" % n)
                al.free()
        rows_alloc.check("rows")
    finally:
        rows_alloc.free()
    if offset == 0:  # the method, on rows [m] and [m, size]
        d_rows, d_src = up(ctx, rows, np.array([500, 1, 7], np.int32))
        out = ctx.gather_rows_i32(d_src, d_rows)
        np.testing.assert_array_equal(out.download(), rows[[499, 0, 6]])
        free(d_rows, d_src, out)


@pytest.mark.gpu
@pytest.mark.parametrize("size", [1, 2])
@pytest.mark.parametrize("offset", [0, 8])
def test_gather_rows_as_doubles_and_as_ints(ctx, size, offset):
    """the one kernel behind both calls: the same buffer gathered as rows of `size` doubles and as rows of 2 size
    ints gives the same bytes.  size 2 at offset 0 moves 16-byte pieces in both; size 2 at offset 8 falls back to
    elements (bases not 16-byte aligned), size 1 is never a multiple of 16 bytes: 8-byte against 4-byte pieces"""
    rng = np.random.default_rng(10 * size + offset)
    rows = rng.integers(-2 ** 31, 2 ** 31 - 1, (70, 2 * size)).astype(np.int32)  # (any bit pattern: NaNs among them)
    d_rows, rows_alloc = device_view(ctx, rows, offset)
    try:
        for n in (0, 1, 65):
            src = rng.integers(1, 71, n).astype(np.int32)
            d_src, src_alloc = device_view(ctx, src, 4)
            d_f64, f64_alloc = device_view(ctx, np.full((n, 2 * size), SENT, np.int32), offset)
            d_i32, i32_alloc = device_view(ctx, np.full((n, 2 * size), SENT, np.int32), offset)
            assert ctx.lib.pmmg_hip_gather_rows(ctx.h, n, P(d_src), size, P(d_rows), P(d_f64)) == 1, ctx.error()
            assert ctx.lib.pmmg_hip_gather_rows_i32(ctx.h, n, P(d_src), 2 * size, P(d_rows), P(d_i32)) == 1, ctx.error()
            as_f64, as_i32 = d_f64.download(), d_i32.download()
            assert as_f64.tobytes() == as_i32.tobytes()
            np.testing.assert_array_equal(as_i32, rows[src - 1])
            for al in (src_alloc, f64_alloc, i32_alloc):
                al.check("n=%d" % n)
                al.free()
        rows_alloc.check("rows")
    finally:
        rows_alloc.free()


# ---------------------------------------------------------------- 7. chains on the device

@pytest.mark.gpu
@pytest.mark.parametrize("name", [("a", True), ("c", False)], ids=str)
def test_split_merge_round_trip(ctx, name):
    """no restatement: split, merge, and the identities of the round trip from the downloaded maps; the adjacency
    that pmmg_hip_build_adjacency builds on tetv_out is the snapshot's definition on it, and the original's renamed"""
    g = R.mesh_case(*name)
    tetv, adja, part = up(ctx, g["tetv"], g["adja"], g["part"])
    sp = ctx.split_groups(g["np"], part, g["ncolor"], tetv=tetv, adja=adja)
    mg = ctx.merge_groups(sp, color=np.arange(g["ncolor"]))
    built, _ = ctx.build_adjacency(mg["np"], mg["tetv_out"], tet8=False)
    try:
        assert (mg["np"], mg["ne"]) == (g["np"], 6000)
        tet = sp["old_tet"].download()[mg["src_tet"].download() - 1]
        pnt = sp["old_pt"].download()[mg["src_pt"].download() - 1]
        tv = mg["tetv_out"].download()
        assert sorted(tet.tolist()) == list(range(1, 6001)) and sorted(pnt.tolist()) == list(range(1, g["np"] + 1))
        np.testing.assert_array_equal(pnt[tv - 1], g["tetv"][tet - 1])
        np.testing.assert_array_equal(mg["mark_out"].download(), g["part"][tet - 1])
        want, non = snapshot_ref.adjacency(tv)
        assert not non
        np.testing.assert_array_equal(built.download(), want)
        merged_of = np.empty(6001, np.int64)
        merged_of[tet] = np.arange(1, 6001)
        a = g["adja"][tet - 1].astype(np.int64)
        np.testing.assert_array_equal(want, np.where(a != 0, 4 * merged_of[a // 4] + a % 4, 0))
        # the marks through gather_rows_i32 are the marks the call wrote
        dcol = ctx.upload(np.repeat(np.arange(g["ncolor"], dtype=np.int32), sp["count"][:, 0]))
        marks = ctx.gather_rows_i32(mg["src_tet"], dcol)
        np.testing.assert_array_equal(marks.download(), mg["mark_out"].download())
        free(dcol, marks)
    finally:
        free(tetv, adja, part, built, *[sp[k] for k in ("old_tet", "new_tet", "tet8_out") + LISTS],
             *[mg[k] for k in OUTS])


def _group_case(ctx, grp, q, pclass, hausd):
    """the oracle's view of one device group: its arrays downloaded, and the queries it was given"""
    t8 = grp["tet8"].download()
    mesh = synth.Mesh(kind=synth.CUBE, n=0, xyz=grp["xyz"].download(), tetv=np.ascontiguousarray(t8[:, :4]),
                      adja=np.ascontiguousarray(t8[:, 4:]), triv=grp["triv"].download(), adjt=grp["adjt"].download(),
                      isbdy=np.zeros(grp["np"], np.uint8))
    met, fields = grp["met"].download(), [f.download() for f in grp["fields"]]
    return dict(B=O.Background(mesh, met, fields, hausd), new=types.SimpleNamespace(xyz=q), pclass=pclass, met=met,
                fields=fields, hausd=hausd)


@pytest.mark.gpu
def test_merge_then_move_then_split_then_transfer(ctx):
    """groups -> merged group -> marks -> moved marks -> fix -> packed colours -> groups -> transfer, all on the
    device: the groups of a split are merged with mark_out as the marks, the interfaces move, the merged group is
    split again and every new group's transfer meets parity.check against the oracle on that group's own arrays"""
    case = make_case(kind=synth.CUBE, n_old=6, n_new=7, with_ref=False)
    bg, new = case["bg"], case["new"]
    slab = lambda x: np.minimum((x * 2).astype(np.int32), 1)
    part0 = slab(bg.xyz[bg.tetv - 1, 0].mean(axis=1))
    tetv, adja, dpart0, dxyz, dmet = up(ctx, bg.tetv, bg.adja, part0, bg.xyz, case["met"])
    dfields = up(ctx, *case["fields"])
    # the iteration's groups, resident
    sp0 = ctx.split_groups(bg.np, dpart0, 2, tetv=tetv, adja=adja)
    _, rows0 = ctx.groups_from_split(sp0, dxyz, dmet, dfields)
    # the merged group
    mg = ctx.merge_groups(sp0, color=[0, 1])
    assert (mg["np"], mg["ne"]) == (bg.np, bg.ne)
    mxyz, mmet, mfields = ctx.merged_from_groups(mg, rows0[0], rows0[1], rows0[2:])
    pnt = sp0["old_pt"].download()[mg["src_pt"].download() - 1]
    np.testing.assert_array_equal(mxyz.download().view(np.uint64), bg.xyz[pnt - 1].view(np.uint64))
    np.testing.assert_array_equal(mmet.download().view(np.uint64), case["met"][pnt - 1].view(np.uint64))
    mtetv, dmark = mg["tetv_out"], mg["mark_out"]
    madja, _ = ctx.build_adjacency(mg["np"], mtetv, tet8=False)
    # marks -> moved marks -> fix -> packed colours
    nelem = sp0["count"][:, 0].astype(np.int32)
    w = nelem + np.array([1, 0], np.int32)
    mark_before = dmark.download()
    color, front = ctx.interface_points(mg["np"], dmark, w, tetv=mtetv)
    res = ctx.move_interfaces(mg["np"], dmark, w, nelem, tetv=mtetv, adja=madja, ptcolor=color, ptfront=front, nlayers=2)
    assert (res["layers_done"], res["blocked"]) == (2, 0) and res["moved"].min() > 0
    dpart, ngrp = ctx.remap_colors(dmark, 2, tetv=mtetv)
    assert ngrp == 2 and (dpart.download() != mark_before).sum() > 0
    # the new groups and their transfer
    sp = ctx.split_groups(mg["np"], dpart, ngrp, tetv=mtetv, adja=madja)
    groups, owned = ctx.groups_from_split(sp, mxyz, mmet, mfields)
    qslab = slab(new.xyz[:, 0])
    keep, queries = [], []
    for g, grp in enumerate(groups):
        q = np.ascontiguousarray(new.xyz[qslab == g])
        pc = np.ascontiguousarray(case["pclass"][qslab == g])
        triv, adjt = ctx.build_boundary(grp["np"], tet8=grp["tet8"])
        grp.update(triv=triv, adjt=adjt, hausd=case["hausd"], xyz_new=ctx.upload(q), pclass=ctx.upload(pc),
                   met_out=ctx.upload(np.full((q.shape[0], 6), np.nan)),
                   fields_out=[ctx.upload(np.full((q.shape[0], f.shape[1]), np.nan)) for f in case["fields"]],
                   elem_out=ctx.upload(np.zeros(q.shape[0], np.int32)), hit_out=ctx.upload(np.zeros(q.shape[0], np.int8)))
        keep += [triv, adjt, grp["xyz_new"], grp["pclass"], grp["met_out"], grp["elem_out"], grp["hit_out"]]
        keep += grp["fields_out"]
        queries.append((q, pc))
    ctx.locate_interp_groups(groups)
    for grp, (q, pc) in zip(groups, queries):
        out = dict(met=grp["met_out"].download(), fields=[f.download() for f in grp["fields_out"]],
                   elem=grp["elem_out"].download(), hit=grp["hit_out"].download())
        rep = check(_group_case(ctx, grp, q, pc, case["hausd"]), out)
        assert rep["n"] == int((pc != 0).sum()) > 0
        print("group", grp["np"], grp["ne"], rep["hits"], "exact", rep["exact"], "of", rep["n"])
    free(tetv, adja, dpart0, dxyz, dmet, *dfields, *rows0, mxyz, mmet, *mfields, madja, color, front, dpart, *owned,
         *keep, *[sp0[k] for k in ("old_tet", "new_tet", "tet8_out") + LISTS],
         *[sp[k] for k in ("old_tet", "new_tet", "tet8_out") + LISTS], *[mg[k] for k in OUTS])


# ---------------------------------------------------------------- 8. the host layer

@pytest.mark.gpu
def test_host_layer(ctx):
    """pmmg_merge_grps from host arrays: the device call's arrays, and the rows gathered through the two maps"""
    g, sp, color, want = mesh_reference(("b", True), True)
    rng = np.random.default_rng(3)
    xyz0, met0, ref0 = rng.random((g["np"], 3)), rng.random((g["np"], 6)), rng.integers(0, 9, 6000).astype(np.int32)
    xyz, met = np.ascontiguousarray(xyz0[sp["old_pt"] - 1]), np.ascontiguousarray(met0[sp["old_pt"] - 1])
    tref = np.ascontiguousarray(ref0[sp["old_tet"] - 1])
    count = np.ascontiguousarray(sp["count"], np.int32)
    cnt = (_native.HipSplitCount * count.shape[0])(*[_native.HipSplitCount(*[int(v) for v in r]) for r in count])
    col = np.ascontiguousarray(color, np.int32)
    lib, res = _native.host_lib(), _native.HostMergeResult()
    hp = lambda a: np.ascontiguousarray(a).ctypes.data_as(ctypes.c_void_p)
    arrays = [np.ascontiguousarray(sp[k], np.int32) for k in ("tetv_out", "node_idx1", "node_idx2", "face_idx1", "face_idx2")]
    ok = lib.pmmg_merge_grps(ctx.h, count.shape[0], cnt, *[hp(a) for a in arrays], sp["nnode_end"], sp["nface_end"],
                             hp(col), hp(xyz), 6, hp(met), hp(tref), ctypes.byref(res))
    assert ok == 1, ctx.error()
    try:
        assert (res.np, res.ne, res.met_size) == (want["np"], want["ne"], 6)
        view = lambda p, n: np.ctypeslib.as_array(p, shape=(n,)).copy() if n else np.zeros(0)
        got = dict(new_pt=view(res.new_pt, xyz.shape[0]), src_pt=view(res.src_pt, res.np), new_tet=view(res.new_tet, 6000),
                   src_tet=view(res.src_tet, 6000), tetv_out=view(res.tetv, 24000), mark_out=view(res.mark, 6000),
                   node_val=view(res.node_val, sp["nnode_end"]), face_val=view(res.face_val, sp["nface_end"]))
        for k, v in got.items():
            np.testing.assert_array_equal(v, want[k].reshape(-1), err_msg=k)
        pnt, tet = sp["old_pt"][want["src_pt"] - 1], sp["old_tet"][want["src_tet"] - 1]
        np.testing.assert_array_equal(view(res.xyz, 3 * res.np).view(np.uint64), xyz0[pnt - 1].reshape(-1).view(np.uint64))
        np.testing.assert_array_equal(view(res.met, 6 * res.np).view(np.uint64), met0[pnt - 1].reshape(-1).view(np.uint64))
        np.testing.assert_array_equal(view(res.tref, 6000), ref0[tet - 1])
    finally:
        lib.pmmg_merge_result_free(ctypes.byref(res))
    assert not res.new_pt and res.np == 0
    # a refusal comes back as 0 with the result zeroed
    arrays[1] = arrays[1].copy()
    arrays[1][0] = 0
    ok = lib.pmmg_merge_grps(ctx.h, count.shape[0], cnt, *[hp(a) for a in arrays], sp["nnode_end"], sp["nface_end"],
                             hp(col), hp(xyz), 6, hp(met), hp(tref), ctypes.byref(res))
    assert ok == 0 and "node index1" in ctx.error() and not res.tetv
