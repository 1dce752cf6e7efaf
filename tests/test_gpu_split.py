"""pmmg_hip_split_groups and pmmg_hip_gather_rows against the restatements of
tests/split_ref.py, exactly (runs on the MI355X).

tests/test_split_ref_host.py shows, on the CPU, that split_par (array
operations) equals split_seq (the reference's loop, transcribed) on the
fixtures; here every output of the device is compared with split_seq, and the
1M-tetra case, where the transcribed loop would take minutes, with split_par.

Every call goes through split(), which puts 256 guard bytes around every
device output and guard words around every host output, pre-fills the outputs
with SENT and checks that nothing beyond a list's length was written."""
import ctypes
import functools

import numpy as np
import pytest

import contig_ref as R
import snapshot_ref
import split_ref as S
from parity import device_view, make_case, run_gpu, same_outputs
from parmmg_amd import _native, synth
from parmmg_amd.transfer import DeviceArray, TransferContext, pack_tet8
from test_gpu_contig import P, SENT, free, guarded, host_guarded, host_unguard, unguard, up
from test_metis_graph import cut, fixture

TET_OUTS = ("new_tet", "tetv_out", "adja_out", "tet8_out")
LISTS = ("old_pt", "face_idx1", "face_idx2", "node_idx1", "node_idx2")
WIDTH = dict(new_tet=1, tetv_out=4, adja_out=4, tet8_out=8)


@pytest.fixture(scope="module")
def ctx():
    with TransferContext(0) as c:
        yield c


def split(ctx, npv, ne, part, ngrp, tetv=None, adja=None, tet8=None, node_pos=None, face_old=None, nnode0=0, nface0=0,
          caps=None, outs=TET_OUTS, want_ok=True, ne_arg=None):
    """the C call with guarded outputs.  caps None: a call with caps of 0 sizes the lists (and must fill the
    counts), then the call with the exact caps.  Returns dict(ok, msg, count [ngrp, 4], nnode_end, nface_end, and
    every output as an array of its allocated length)."""
    def once(caps_):
        bufs = {k: guarded(ctx, np.full(ne * WIDTH.get(k, 1), SENT)) for k in ("old_tet",) + tuple(outs)}
        lens = dict(old_pt=caps_[0], face_idx1=caps_[1], face_idx2=caps_[1], node_idx1=caps_[2], node_idx2=caps_[2])
        bufs.update({k: guarded(ctx, np.full(lens[k], SENT)) for k in LISTS})
        cw, cp = host_guarded(4 * ngrp)
        ew, ep = host_guarded(2)
        d = lambda k: P(bufs[k][1]) if k in bufs else None
        ok = ctx.lib.pmmg_hip_split_groups(
            ctx.h, npv, ne if ne_arg is None else ne_arg, P(tetv), P(adja), P(tet8), P(part), ngrp, P(node_pos),
            P(face_old), nnode0, nface0, ctypes.cast(cp, ctypes.POINTER(_native.HipSplitCount)), caps_[0], caps_[1],
            caps_[2], d("old_tet"), d("new_tet"), d("tetv_out"), d("adja_out"), d("tet8_out"), d("old_pt"),
            d("face_idx1"), d("face_idx2"), d("node_idx1"), d("node_idx2"),
            ctypes.cast(ep, ctypes.POINTER(ctypes.c_int)),
            ctypes.cast(ctypes.c_void_p(ep.value + 4), ctypes.POINTER(ctypes.c_int)))
        out = dict(ok=ok, msg=ctx.error(), count=host_unguard(cw, 4 * ngrp).reshape(ngrp, 4))
        out["nnode_end"], out["nface_end"] = host_unguard(ew, 2).tolist()
        for k, (buf, view) in bufs.items():
            out[k] = unguard(buf, view.shape[0])
        return out

    if caps is None:
        sized = once((0, 0, 0))
        if want_ok and ne:
            assert sized["ok"] == 0 and "cap" in sized["msg"], sized["msg"]
            assert sized["count"][:, 0].sum() == ne
            assert all((sized[k].size == 0) for k in LISTS)
        caps = [int(sized["count"][:, c].sum()) for c in (1, 2, 3)] if sized["count"].min() >= 0 else (0, 0, 0)
    out = once(caps)
    if want_ok:
        assert out["ok"] == 1, out["msg"]
        print("ne", ne, "ngrp", ngrp, "totals", out["count"].sum(axis=0).tolist(), "rounds",
              ctx.lib.pmmg_hip_split_rounds(ctx.h))
    return out


def assert_split(got, want, outs=TET_OUTS):
    """every output equal to the restatement's; nothing written beyond a list's length"""
    np.testing.assert_array_equal(got["count"], want["count"])
    assert (got["nnode_end"], got["nface_end"]) == (want["nnode_end"], want["nface_end"])
    np.testing.assert_array_equal(got["old_tet"], want["old_tet"])
    tet8 = np.hstack([want["tetv_out"], want["adja_out"]]).reshape(-1)
    flat = dict(new_tet=want["new_tet"], tetv_out=want["tetv_out"].reshape(-1), adja_out=want["adja_out"].reshape(-1),
                tet8_out=tet8)
    for k in outs:
        np.testing.assert_array_equal(got[k], flat[k], err_msg=k)
    for k in LISTS:
        n = want[k].size
        np.testing.assert_array_equal(got[k][:n], want[k], err_msg=k)
        assert (got[k][n:] == SENT).all(), k


def run_case(ctx, tetv, adja, part, ngrp, npv, ref=S.split_seq, **kw):
    tetv, adja, part = (np.ascontiguousarray(a, np.int32) for a in (tetv, adja, part))
    want = ref(tetv, adja, part, ngrp, npv, **kw)
    dev = up(ctx, tetv, adja, part, kw.get("node_pos"), kw.get("face_old"))
    try:
        got = split(ctx, npv, tetv.shape[0], dev[2], ngrp, tetv=dev[0], adja=dev[1], node_pos=dev[3], face_old=dev[4],
                    nnode0=kw.get("nnode0", 0), nface0=kw.get("nface0", 0))
        assert_split(got, want)
    finally:
        free(*dev)
    return got, want


# ---------------------------------------------------------------- 1. edges

@pytest.mark.gpu
def test_one_tetra(ctx):
    got, _ = run_case(ctx, [[3, 1, 4, 2]], np.zeros((1, 4)), [0], 1, 4)
    assert got["count"].tolist() == [[1, 4, 0, 0]] and got["tetv_out"].tolist() == [1, 2, 3, 4]
    assert got["old_pt"].tolist() == [3, 1, 4, 2]


@pytest.mark.gpu
def test_two_tetra_two_groups(ctx):
    """one interface face; both iploc sides by hand"""
    tetv = np.array([[1, 2, 3, 4], [3, 2, 5, 4]], np.int32)  # share {2, 3, 4}: face 0 of the first, face 2 of the second
    adja, non = snapshot_ref.adjacency(tetv)
    assert not non and adja.tolist() == [[4 * 2 + 2, 0, 0, 0], [0, 0, 4 * 1 + 0, 0]]
    got, _ = run_case(ctx, tetv, adja, [0, 1], 2, 5, nface0=10, nnode0=100)
    assert got["count"].tolist() == [[1, 4, 1, 3], [1, 4, 1, 3]]
    # the owner (colour 0): tetra 1, face 0, iploc 0 names v[idir[0][0]] = vertex 2; the other side: tetra 1 of its
    # group, face 2 = (v0, v1, v3) = (3, 2, 4): vertex 2 is at position 1
    assert got["face_idx1"].tolist() == [12 * 1 + 3 * 0 + 0, 12 * 1 + 3 * 2 + 1]
    assert got["face_idx2"].tolist() == [10, 10] and got["nface_end"] == 11
    # nodes: group 0 gives 2, 3, 4 (new ids 2, 3, 4) the positions 101..103; group 1 lists them first (its new ids
    # of 3, 2, 4 are 1, 2, 4, in ascending new id)
    assert got["node_idx1"].tolist() == [2, 3, 4, 1, 2, 4] and got["node_idx2"].tolist() == [101, 102, 103, 102, 101, 103]
    assert got["nnode_end"] == 106  # nitem counts entries, not nodes
    assert got["adja_out"].tolist() == [0] * 8


@pytest.mark.gpu
def test_empty_colours(ctx):
    g = R.mesh_case("a", False)
    part = np.ones(6000, np.int32)
    got, _ = run_case(ctx, g["tetv"], g["adja"], part, 3, g["np"])
    assert got["count"][:, 0].tolist() == [0, 6000, 0] and got["count"][[0, 2]].sum() == 0
    np.testing.assert_array_equal(got["adja_out"].reshape(-1, 4), g["adja"])


@pytest.mark.gpu
def test_every_tetra_a_group(ctx):
    bg, _ = fixture()
    m = 320
    a = np.ascontiguousarray(cut(bg.adja, np.arange(bg.ne) < m)[:m])
    part = np.random.default_rng(4).permutation(m).astype(np.int32)
    got, _ = run_case(ctx, bg.tetv[:m], a, part, m, bg.np)
    assert (got["count"][:, :2] == [1, 4]).all() and (got["adja_out"] == 0).all()


@pytest.mark.gpu
@pytest.mark.parametrize("m", [63, 64, 65, 255, 256, 257, 4097])
def test_sizes(ctx, m):
    """the wave, block and scan-chunk edges: a prefix of the lattice, two colours alternating per tetra"""
    bg, _ = fixture()
    npv, tetv = snapshot_ref.prefix((bg.np, bg.tetv), m)
    adja, non = snapshot_ref.adjacency(tetv)
    assert not non
    run_case(ctx, tetv, adja, np.arange(m) % 2, 2, npv)


@pytest.mark.gpu
def test_no_tetra(ctx):
    got = split(ctx, 5, 0, None, 3)
    assert got["ok"] == 1 and (got["count"] == 0).all() and (got["nnode_end"], got["nface_end"]) == (0, 0)


# ---------------------------------------------------------------- 2. the fixtures, on every layout

@functools.lru_cache(maxsize=None)
def mesh_reference(name, old):
    g = R.mesh_case(*name)
    kw = {}
    if old:
        node_pos, face_old, nnode0, nface0 = S.old_positions(g["tetv"], g["adja"], 7)
        kw = dict(node_pos=node_pos, face_old=face_old, nnode0=nnode0, nface0=nface0)
    return g, kw, S.split_seq(g["tetv"], g["adja"], g["part"], g["ncolor"], g["np"], **kw)


@pytest.mark.gpu
@pytest.mark.parametrize("name", R.MESH_CASES, ids=str)
def test_mesh_fixtures(ctx, name):
    g, _, want = mesh_reference(name, False)
    _, kw, want_old = mesh_reference(name, True)
    ne, ngrp, npv = 6000, g["ncolor"], g["np"]
    tetv, adja, tet8, part, npos, fold = up(ctx, g["tetv"], g["adja"], pack_tet8(g["tetv"], g["adja"]), g["part"],
                                            kw["node_pos"], kw["face_old"])
    try:
        a = split(ctx, npv, ne, part, ngrp, tetv=tetv, adja=adja)
        b = split(ctx, npv, ne, part, ngrp, tet8=tet8)
        c = split(ctx, npv, ne, part, ngrp, tet8=tet8, outs=("tet8_out",))
        assert_split(a, want)
        assert_split(c, want, outs=("tet8_out",))
        for k in ("old_tet", "count") + TET_OUTS + LISTS:
            assert a[k].tobytes() == b[k].tobytes(), k
            if k in c:
                assert a[k].tobytes() == c[k].tobytes(), k
        d = split(ctx, npv, ne, part, ngrp, tetv=tetv, adja=adja, node_pos=npos, face_old=fold, nnode0=kw["nnode0"],
                  nface0=kw["nface0"])
        assert_split(d, want_old)
        for k in ("old_tet",) + TET_OUTS + ("old_pt",):  # the old positions change the lists only
            assert a[k].tobytes() == d[k].tobytes(), k
    finally:
        free(tetv, adja, tet8, part, npos, fold)


@pytest.mark.gpu
@pytest.mark.parametrize("ngrp", [1000, 6000])
def test_many_colours(ctx, ngrp):
    """beyond one digit of the colour sort; most colours of 6000 are empty or a single tetra"""
    g = R.mesh_case("a", True)
    part = np.random.default_rng(ngrp).integers(0, ngrp, 6000).astype(np.int32)
    run_case(ctx, g["tetv"], g["adja"], part, ngrp, g["np"])


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


@pytest.mark.gpu
@pytest.mark.parametrize("numbering", ["lattice", "mmg"])
def test_one_million_tetra(ctx, numbering):
    tetv, adja, part, npv = big(numbering)
    got, want = run_case(ctx, tetv, adja, part, 16, npv, ref=S.split_par)
    assert got["count"][:, 0].min() > 0 and got["nface_end"] > 0


# ---------------------------------------------------------------- 4. caps, refusals

@pytest.mark.gpu
def test_caps(ctx):
    g, _, want = mesh_reference(("b", True), False)
    tot = [int(want["count"][:, c].sum()) for c in (1, 2, 3)]
    tetv, adja, part = up(ctx, g["tetv"], g["adja"], g["part"])
    try:
        for short in range(3):
            caps = list(tot)
            caps[short] -= 1
            got = split(ctx, g["np"], 6000, part, g["ncolor"], tetv=tetv, adja=adja, caps=caps, want_ok=False)
            assert got["ok"] == 0 and "cap" in got["msg"], got["msg"]
            np.testing.assert_array_equal(got["count"], want["count"])
            assert (got["nnode_end"], got["nface_end"]) == (want["nnode_end"], want["nface_end"])
            for k in LISTS:
                assert (got[k] == SENT).all(), k
        assert_split(split(ctx, g["np"], 6000, part, g["ncolor"], tetv=tetv, adja=adja), want)  # sized by caps of 0
        roomy = split(ctx, g["np"], 6000, part, g["ncolor"], tetv=tetv, adja=adja, caps=[t + 5 for t in tot])
        assert_split(roomy, want)
    finally:
        free(tetv, adja, part)


@pytest.mark.gpu
@pytest.mark.parametrize("what", ["part ngrp", "part -1", "unused tetra", "link 3", "link 4ne+4", "vertex np+1", "2^29"])
def test_refusals(ctx, what):
    """each returns 0 with its message and every output still the fill value"""
    g = R.mesh_case("a", False)
    ne, ngrp, npv = 6000, g["ncolor"], g["np"]
    tv, a, colours = np.array(g["tetv"]), np.array(g["adja"]), np.array(g["part"])
    word, ne_arg = "adja", None
    if what.startswith("part"):
        colours[4100], word = (ngrp if what == "part ngrp" else -1), "part"
    elif what == "unused tetra":
        tv[300, 0], word = 0, "unused"
    elif what.startswith("link"):
        a[2571, 2] = 3 if what == "link 3" else 4 * ne + 4
    elif what == "vertex np+1":
        tv[5999, 3], word = npv + 1, "vertex"
    else:
        ne_arg, word = 1 << 29, "2^29"
    tetv, adja, part = up(ctx, tv, a, colours)
    try:
        got = split(ctx, npv, ne, part, ngrp, tetv=tetv, adja=adja, caps=(4 * ne, 4 * ne, 4 * ne), want_ok=False,
                    ne_arg=ne_arg)
        assert got["ok"] == 0 and word in got["msg"], got["msg"]
        for k in ("old_tet",) + TET_OUTS + LISTS:
            assert (got[k] == SENT).all(), k
    finally:
        free(tetv, adja, part)


# ---------------------------------------------------------------- 5. determinism, isolation, the device's own check

@pytest.mark.gpu
def test_two_calls_and_release_scratch(ctx):
    g, kw, want = mesh_reference(("c", True), True)
    dev = up(ctx, g["tetv"], g["adja"], g["part"], kw["node_pos"], kw["face_old"])
    args = dict(tetv=dev[0], adja=dev[1], node_pos=dev[3], face_old=dev[4], nnode0=kw["nnode0"], nface0=kw["nface0"])
    try:
        a = split(ctx, g["np"], 6000, dev[2], g["ncolor"], **args)
        b = split(ctx, g["np"], 6000, dev[2], g["ncolor"], **args)
        ctx.release_scratch()
        c = split(ctx, g["np"], 6000, dev[2], g["ncolor"], **args)
        assert_split(a, want)
        for k in ("old_tet", "count") + TET_OUTS + LISTS:
            assert a[k].tobytes() == b[k].tobytes() == c[k].tobytes(), k
    finally:
        free(*dev)


@pytest.mark.gpu
def test_transfer_does_not_see_the_split_scratch():
    g, _, want = mesh_reference(("b", False), False)
    case = make_case(kind=synth.CUBE, n_old=6, n_new=7, with_ref=False)
    with TransferContext(0) as c:
        before = run_gpu(case, ctx=c)
        tetv, adja, part = up(c, g["tetv"], g["adja"], g["part"])
        assert_split(split(c, g["np"], 6000, part, g["ncolor"], tetv=tetv, adja=adja), want)
        after = run_gpu(case, ctx=c)
        free(tetv, adja, part)
    same_outputs(before, run_gpu(case))
    same_outputs(before, after)


@pytest.mark.gpu
@pytest.mark.parametrize("name", [("a", True), ("c", False)], ids=str)
def test_groups_adjacency_built_on_the_device(ctx, name):
    """no restatement: pmmg_hip_build_adjacency on each group's tetv_out gives that group's adja_out"""
    g = R.mesh_case(*name)
    tetv, adja, part = up(ctx, g["tetv"], g["adja"], g["part"])
    sp = ctx.split_groups(g["np"], part, g["ncolor"], tetv=tetv, adja=adja, want=("tetv_out", "adja_out"))
    try:
        want = sp["adja_out"].download()
        for grp in range(g["ncolor"]):
            t0, t1 = int(sp["te_off"][grp]), int(sp["te_off"][grp + 1])
            view = DeviceArray(sp["tetv_out"].ptr + 16 * t0, 16 * (t1 - t0), (t1 - t0, 4), np.dtype(np.int32), ctx)
            built, _ = ctx.build_adjacency(int(sp["count"][grp, 1]), view, tet8=False)
            np.testing.assert_array_equal(built.download(), want[t0:t1])
            built.free()
    finally:
        free(tetv, adja, part, *[sp[k] for k in ("old_tet", "tetv_out", "adja_out") + LISTS])


# ---------------------------------------------------------------- 6. gather_rows

@pytest.mark.gpu
@pytest.mark.parametrize("size", [1, 3, 6])
@pytest.mark.parametrize("offset", [0, 8])
def test_gather_rows(ctx, size, offset):
    rng = np.random.default_rng(size)
    rows = rng.random((500, size))
    d_rows, rows_alloc = device_view(ctx, rows, offset)
    try:
        for n in (0, 1, 63, 64, 65, 4097):
            src = rng.integers(1, 501, n).astype(np.int32)  # (with repeats)
            d_src, src_alloc = device_view(ctx, src, 4)
            d_out, out_alloc = device_view(ctx, np.full((n, size), np.nan), offset)
            ok = ctx.lib.pmmg_hip_gather_rows(ctx.h, n, P(d_src), size, P(d_rows), P(d_out))
            assert ok == 1, ctx.error()
            np.testing.assert_array_equal(d_out.download(), rows[src - 1])
            for al in (src_alloc, out_alloc):
                al.check("gather_rows n=%d" % n)
                al.free()
        rows_alloc.check("rows")
    finally:
        rows_alloc.free()


# ---------------------------------------------------------------- 7. end to end: split, gather, transfer

def _outputs(ctx, groups):
    out = []
    for g in groups:
        out.append(dict(met=g["met_out"].download(), fields=[f.download() for f in g["fields_out"]],
                        elem=g["elem_out"].download(), hit=g["hit_out"].download()))
    return out


@pytest.mark.gpu
def test_split_then_transfer(ctx):
    """the background of the small case cut into 4 slabs on the device, its rows gathered there, and the new points
    of each slab transferred against their group: bit-identical to the same call on groups cut by split_seq and
    numpy on the host; the host layer's pmmg_split_grps gives the same arrays"""
    case = make_case(kind=synth.CUBE, n_old=6, n_new=7, with_ref=False)
    bg, new = case["bg"], case["new"]
    slab = lambda x: np.minimum((x * 4).astype(np.int32), 3)
    part = slab(bg.xyz[bg.tetv - 1, 0].mean(axis=1))
    qslab = slab(new.xyz[:, 0])
    want = S.split_seq(bg.tetv, bg.adja, part, 4, bg.np)
    te, pt, _, _ = S.segments(want)
    rows = [bg.xyz, case["met"]] + list(case["fields"])
    # on the device
    tetv, adja, dpart, dxyz, dmet = up(ctx, bg.tetv, bg.adja, part, bg.xyz, case["met"])
    dfields = up(ctx, *case["fields"])
    sp = ctx.split_groups(bg.np, dpart, 4, tetv=tetv, adja=adja)
    dev_groups, owned = ctx.groups_from_split(sp, dxyz, dmet, dfields)
    np.testing.assert_array_equal(sp["count"], want["count"])
    np.testing.assert_array_equal(sp["tet8_out"].download(), np.hstack([want["tetv_out"], want["adja_out"]]))
    for k in LISTS:
        np.testing.assert_array_equal(sp[k].download(), want[k], err_msg=k)
    for arr, src in zip(owned, rows):
        np.testing.assert_array_equal(arr.download().view(np.uint64), src[want["old_pt"] - 1].view(np.uint64))
    # on the host
    host_groups = []
    for g in range(4):
        tv, ad = want["tetv_out"][te[g]:te[g + 1]], want["adja_out"][te[g]:te[g + 1]]
        old = want["old_pt"][pt[g]:pt[g + 1]] - 1
        host_groups.append(dict(np=old.size, ne=tv.shape[0], xyz=ctx.upload(bg.xyz[old]),
                                tet8=ctx.upload(pack_tet8(tv, ad)), met=ctx.upload(case["met"][old]),
                                fields=[ctx.upload(f[old]) for f in case["fields"]]))
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
    for a, b in zip(_outputs(ctx, dev_groups), _outputs(ctx, host_groups)):
        same_outputs(a, b)
        assert (a["hit"] != 0).sum() > 0
    for grp in host_groups:
        keep += [grp["xyz"], grp["tet8"], grp["met"]] + grp["fields"]
    free(tetv, adja, dpart, dxyz, dmet, *dfields, *owned, *keep,
         *[sp[k] for k in ("old_tet", "new_tet", "tet8_out") + LISTS])
    # the host layer
    lib = _native.host_lib()
    vp = lambda arr: arr.ctypes.data_as(ctypes.c_void_p)
    res = _native.HostSplitResult()
    fs = [np.ascontiguousarray(f) for f in case["fields"]]
    sizes = np.array([f.shape[1] for f in fs], np.int32)
    ptrs = (ctypes.c_void_p * len(fs))(*[f.ctypes.data for f in fs])
    ok = lib.pmmg_split_grps(ctx.h, bg.np, vp(bg.xyz), bg.ne, vp(bg.tetv), vp(bg.adja), vp(part), 4, 6, vp(case["met"]),
                             len(fs), vp(sizes), ctypes.cast(ptrs, ctypes.c_void_p), None, None, 0, 0, ctypes.byref(res))
    assert ok == 1, ctx.error()
    try:
        arr = lambda p, n, t=np.int32: np.ctypeslib.as_array(p, shape=(n,)).astype(t) if n else np.zeros(0, t)
        npt = int(want["count"][:, 1].sum())
        assert (res.npt, res.nface, res.nnode) == tuple(int(want["count"][:, c].sum()) for c in (1, 2, 3))
        assert (res.nnode_end, res.nface_end) == (want["nnode_end"], want["nface_end"])
        np.testing.assert_array_equal(arr(res.old_tet, bg.ne), want["old_tet"])
        np.testing.assert_array_equal(arr(res.new_tet, bg.ne), want["new_tet"])
        np.testing.assert_array_equal(arr(res.tetv, 4 * bg.ne), want["tetv_out"].reshape(-1))
        np.testing.assert_array_equal(arr(res.adja, 4 * bg.ne), want["adja_out"].reshape(-1))
        np.testing.assert_array_equal(arr(res.old_pt, npt), want["old_pt"])
        for k in LISTS[1:]:
            np.testing.assert_array_equal(arr(getattr(res, k), want[k].size), want[k], err_msg=k)
        old = want["old_pt"] - 1
        np.testing.assert_array_equal(arr(res.xyz, 3 * npt, np.float64), bg.xyz[old].reshape(-1))
        np.testing.assert_array_equal(arr(res.met, 6 * npt, np.float64), case["met"][old].reshape(-1))
        for i, f in enumerate(fs):
            np.testing.assert_array_equal(arr(res.fields[i], f.shape[1] * npt, np.float64), f[old].reshape(-1))
        got_count = np.array([(res.count[g].ne, res.count[g].np, res.count[g].nface, res.count[g].nnode) for g in range(4)])
        np.testing.assert_array_equal(got_count, want["count"])
    finally:
        lib.pmmg_split_result_free(ctypes.byref(res))
