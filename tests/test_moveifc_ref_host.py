"""The two restatements of the interface displacement (tests/moveifc_ref.py)
against each other and against fixtures worked by hand (CPU only).

ifc_seq is the reference's loop with its fields; ifc_par is the definition of
include/parmmg_hip.h that the device computes.  They are equal wherever no
brake fires and every vertex star is face-connected; where the definition
reports a layer as blocked, the loop really abandons a ball in that layer,
and where it does not, the loop abandons none."""
import ctypes
import functools
import os
import re
import subprocess

import numpy as np
import pytest

import contig_ref as R
import moveifc_ref as M
from parmmg_amd import build

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LAYERS = (1, 2, 4)


def set_points(g):
    """every 7th point of the mesh with the colour of the next colour up: (set_pt, set_color)"""
    pts = np.arange(3, g["np"], 7, dtype=np.int32)
    color, _ = M.seed_par(g["tetv"], g["part"], np.ones(g["ncolor"], np.int32), g["np"])
    return pts, ((color[pts - 1] + 1) % g["ncolor"]).astype(np.int32)


def nelem_of(g, local):
    n = np.bincount(g["part"], minlength=g["ncolor"]).astype(np.int32)
    return n if local else np.full(g["ncolor"], -1, np.int32)


@functools.lru_cache(maxsize=None)
def seq(case, wkind, with_set, local, side_tie="lowest"):
    g = R.mesh_case(*case)
    w = M.weight_table(wkind, g["part"], g["ncolor"])
    nelem = nelem_of(g, local)
    sp, sc = set_points(g) if with_set else (None, None)
    return M.ifc_seq(g["tetv"], g["adja"], g["part"], w, nelem, M.nemin_of(nelem), g["np"], max(LAYERS), sp, sc, side_tie)


@pytest.mark.parametrize("case", R.MESH_CASES, ids=str)
def test_every_star_of_the_fixtures_is_face_connected(case):
    g = R.mesh_case(*case)
    assert M.stars_face_connected(g["tetv"], g["adja"])


@pytest.mark.parametrize("local", [False, True], ids=["foreign", "local"])
@pytest.mark.parametrize("with_set", [False, True], ids=["noset", "set"])
@pytest.mark.parametrize("wkind", M.WEIGHTS)
@pytest.mark.parametrize("case", R.MESH_CASES, ids=str)
def test_definition_equals_the_loop(case, wkind, with_set, local):
    g = R.mesh_case(*case)
    w = M.weight_table(wkind, g["part"], g["ncolor"])
    nelem = nelem_of(g, local)
    sp, sc = set_points(g) if with_set else (None, None)
    want = seq(case, wkind, with_set, local)
    got = M.ifc_par(g["tetv"], g["part"], w, nelem, M.nemin_of(nelem), g["np"], max(LAYERS), sp, sc)
    if not local:
        assert got["blocked"] == 0 and got["layers_done"] == max(LAYERS)
    for n in LAYERS:
        if n > got["layers_done"]:
            break
        a, b = got["layers"][n - 1], want[n - 1]
        for key in ("mark", "color", "front", "nelem"):
            np.testing.assert_array_equal(a[key], b[key], err_msg=f"{key} after {n} layers")
        assert [l["moved"] for l in got["layers"][:n]] == [l["moved"] for l in want[:n]]
    assert all(l["abandoned"] == 0 for l in want[:got["layers_done"]])
    if got["blocked"]:
        assert want[got["layers_done"]]["abandoned"] > 0
    print(case, wkind, "layers done", got["layers_done"], "moved", [l["moved"] for l in got["layers"]])
    assert got["layers_done"] == 0 or got["layers"][0]["moved"] > 0


def test_the_seed_of_the_definition_is_the_seed_of_the_loop():
    for case in R.MESH_CASES:
        g = R.mesh_case(*case)
        for wkind in M.WEIGHTS:
            w = M.weight_table(wkind, g["part"], g["ncolor"])
            st = M.seed_seq(g["tetv"], g["part"], w, g["np"])
            color, front = M.seed_par(g["tetv"], g["part"], w, g["np"])
            np.testing.assert_array_equal(color, st["tmp"][1:])
            np.testing.assert_array_equal(front, [f == st["bf"] for f in st["flag"][1:]])
            assert 0 < front.sum() < g["np"]


@pytest.mark.parametrize("wkind", ["perm", "counts"])
@pytest.mark.parametrize("case", R.MESH_CASES, ids=str)
def test_bfs_and_lowest_agree_without_ties(case, wkind):
    g = R.mesh_case(*case)
    w = M.weight_table(wkind, g["part"], g["ncolor"])
    assert np.unique(w).size == w.size
    a, b = seq(case, wkind, False, False, "bfs"), seq(case, wkind, False, False, "lowest")
    for la, lb in zip(a, b):
        for key in ("mark", "color", "front"):
            np.testing.assert_array_equal(la[key], lb[key])


def tie_differences():
    """{case: (points whose colour differs, tetra whose mark differs)} after 4 layers, bfs against lowest"""
    out = {}
    for case in R.MESH_CASES:
        a, b = seq(case, "ties", False, False, "bfs")[-1], seq(case, "ties", False, False, "lowest")[-1]
        out[case] = (int((a["color"] != b["color"]).sum()), int((a["mark"] != b["mark"]).sum()))
    return out


def test_bfs_and_lowest_differ_with_ties():
    """the counts DESIGN.md §13 records"""
    d = tie_differences()
    print("tie differences (points, tetra) after 4 layers:", d)
    assert any(p > 0 for p, _ in d.values())
    text = open(os.path.join(ROOT, "DESIGN.md")).read()
    sec = text[text.index("## 13."):]
    for (c, s), (p, t) in d.items():
        row = f"| {c} {'scrambled' if s else 'lattice'} | {p} | {t} |"
        assert row in sec, row


# ---------------------------------------------------------------- fixtures worked by hand

def both(tetv, adja, mark, w, nelem, nemin, np_, nlayers, **kw):
    s = M.ifc_seq(tetv, adja, mark, w, nelem, nemin, np_, nlayers, **kw)
    p = M.ifc_par(tetv, mark, w, nelem, nemin, np_, nlayers, **kw)
    return s, p


def test_seed_first_corner_two_tetra():
    """tetra 1 = (1, 2, 3, 4), tetra 2 = (2, 3, 4, 5).  The shared points meet tetra 1 first.  When tetra 2's colour
    wins they change colour once: front.  When tetra 1's colour wins they never change: interface points, not front."""
    tetv, _, np_ = M.path_mesh(2)
    mark = np.array([0, 1], np.int32)
    for seed in (lambda w: M.seed_par(tetv, mark, w, np_),
                 lambda w: (lambda st: (st["tmp"][1:], [f == st["bf"] for f in st["flag"][1:]]))(M.seed_seq(tetv, mark, w, np_))):
        color, front = seed(np.array([2, 1], np.int32))
        assert list(color) == [0, 1, 1, 1, 1] and list(front) == [0, 1, 1, 1, 0]
        color, front = seed(np.array([1, 2], np.int32))
        assert list(color) == [0, 0, 0, 0, 1] and list(front) == [0, 0, 0, 0, 0]
        color, front = seed(np.array([2, 2], np.int32))  # equal weights: nobody beats anybody
        assert list(color) == [0, 0, 0, 0, 1] and list(front) == [0, 0, 0, 0, 0]


def test_seed_and_one_layer_four_tetra():
    """a path of tetra k = (k, k + 1, k + 2, k + 3), marks 1 0 2 0, weights w0 = 3, w1 = 1, w2 = 2.  Points 1 - 4 meet
    colour 1 (the least weight) at their first corner: not front.  Point 5 meets 0, 2, 0: colour 2, front.  Point 6
    meets 2 first.  The layer: point 5 re-marks tetra 2 and 4; their points off the front join it, and point 7
    alone takes the colour (1 beats 2 at points 2 - 4, point 6 has it)."""
    tetv, adja, np_ = M.path_mesh(4)
    mark, w = np.array([1, 0, 2, 0], np.int32), np.array([3, 1, 2], np.int32)
    none = np.full(3, -1, np.int32)
    color, front = M.seed_par(tetv, mark, w, np_)
    assert list(color) == [1, 1, 1, 1, 2, 2, 0] and list(front) == [0, 0, 0, 0, 1, 0, 0]
    s, p = both(tetv, adja, mark, w, none, none * 0, np_, 1)
    for r in (s[0], p["layers"][0]):
        assert list(r["mark"]) == [1, 2, 2, 2] and r["moved"] == 2
        assert list(r["color"]) == [1, 1, 1, 1, 2, 2, 2] and list(r["front"]) == [0, 1, 1, 1, 0, 1, 1]


def test_intermediate_event_decrements_a_colour_that_never_gained():
    """one tetra of colour 0, w = 3 2 1, points 1 and 2 made front with colours 1 and 2: point 1 re-marks the tetra
    to 1 (colour 0 loses one), point 2 re-marks it to 2 and colour 1 loses one it never had"""
    tetv, adja, np_ = M.path_mesh(1)
    mark, w = np.array([0], np.int32), np.array([3, 2, 1], np.int32)
    nelem, nemin = np.array([10, 10, 10], np.int32), np.array([6, 6, 6], np.int32)
    kw = dict(set_pt=np.array([1, 2], np.int32), set_color=np.array([1, 2], np.int32))
    s, p = both(tetv, adja, mark, w, nelem, nemin, np_, 1, **kw)
    for r in (s[0], p["layers"][0]):
        assert list(r["mark"]) == [2] and list(r["nelem"]) == [9, 9, 10] and r["moved"] == 1
        assert list(r["front"]) == [1, 1, 1, 1]  # both events' points are side points, 3 and 4 join
        assert list(r["color"]) == [2, 2, 2, 2]


def test_pinched_star_ball_against_star():
    """tetra 1 = (1, 2, 3, 4) and tetra 2 = (4, 5, 6, 7) share point 4 and no face.  Point 4 takes tetra 2's colour
    and its handle; the reference's ball from there is tetra 2 alone, the module's star is both."""
    tetv = np.array([[1, 2, 3, 4], [4, 5, 6, 7]], np.int32)
    adja = np.zeros((2, 4), np.int32)
    assert not M.stars_face_connected(tetv, adja)
    mark, w = np.array([0, 1], np.int32), np.array([2, 1], np.int32)
    none = np.full(2, -1, np.int32)
    ball = M.ifc_seq(tetv, adja, mark, w, none, none * 0, 7, 1)[0]
    star = M.ifc_seq(tetv, adja, mark, w, none, none * 0, 7, 1, ball="star")[0]
    par = M.ifc_par(tetv, mark, w, none, none * 0, 7, 1)["layers"][0]
    assert list(ball["mark"]) == [0, 1] and ball["moved"] == 0
    assert list(star["mark"]) == [1, 1] and list(par["mark"]) == [1, 1]
    for key in ("color", "front"):
        np.testing.assert_array_equal(star[key], par[key])
    assert list(par["front"]) == [1, 1, 1, 0, 0, 0, 0]


def brake_fixture():
    """a path of 40 tetra in bands of 10, colours 0 1 0 1, colour 0 wins: (args, D[1] of the first layer)"""
    tetv, adja, np_ = M.path_mesh(40)
    mark, w = M.bands(40, 10, 2), np.array([1, 2], np.int32)
    color, front = M.seed_par(tetv, mark, w, np_)
    D = M.layer_par(tetv, mark, w, np.array([-1, -1]), np.array([0, 0]), color, front)["D"]
    return (tetv, adja, mark, w, np_), int(D[1])


def test_brake_at_the_threshold_and_one_past_it():
    (tetv, adja, mark, w, np_), d = brake_fixture()
    assert d > 0
    nemin = np.array([6, 6], np.int32)
    s, p = both(tetv, adja, mark, w, np.array([20, d + 6], np.int32), nemin, np_, 1)  # D == negrp - nemin
    assert p["blocked"] == 0 and s[0]["abandoned"] == 0
    assert list(p["layers"][0]["nelem"]) == [20, 6] == list(s[0]["nelem"])
    np.testing.assert_array_equal(p["layers"][0]["mark"], s[0]["mark"])
    s, p = both(tetv, adja, mark, w, np.array([20, d + 5], np.int32), nemin, np_, 1)  # one larger
    assert p["blocked"] == 1 and p["layers_done"] == 0 and p["layers"] == []
    assert s[0]["abandoned"] >= 1 and s[0]["nelem"][1] == 6  # the loop stopped in the middle of a ball


def test_remap_is_the_packing_of_the_reference():
    """colours 5 and 2 present of 6, the caller's order starting at colour 4 (rank 1 of 3 ranks, two groups each:
    4, 5, 0, 1, 2, 3): colour 5 becomes 0, colour 2 becomes 1"""
    tetv, _, _ = M.path_mesh(5)
    mark = np.array([5, 2, 5, 2, 2], np.int32)
    order = np.array([2, 3, 4, 5, 0, 1], np.int32)
    part, ngrp = M.remap(tetv, mark, 6, order)
    assert list(part) == [0, 1, 0, 1, 1] and ngrp == 2


# ---------------------------------------------------------------- the new exports

NEW_HIP = ["pmmg_hip_ifc_seed", "pmmg_hip_ifc_layers", "pmmg_hip_remap_colors"]


def test_the_new_entry_points_are_declared_and_exported():
    hdr = open(os.path.join(ROOT, "include", "parmmg_hip.h")).read()
    assert "Interface displacement" in hdr
    assert int(re.search(r"#define PMMG_HIP_ABI_VERSION (\d+)", hdr).group(1)) == 6
    nm = lambda so: subprocess.run(["nm", "-D", "--defined-only", so], stdout=subprocess.PIPE, text=True, check=True).stdout
    hip, host = nm(build.HIP_SO), nm(build.HOST_SO)
    for n in NEW_HIP:
        assert re.search(rf"\b{n}\s*\(", hdr), n
        assert re.search(rf"\b{n}$", hip, re.M), n
        getattr(ctypes.CDLL(build.HIP_SO), n)
    assert re.search(r"\bpmmg_part_move_interfaces$", host, re.M)
    from parmmg_amd import _native
    from parmmg_amd.transfer import TransferContext

    assert all(n in _native.HIP_API for n in NEW_HIP) and "pmmg_part_move_interfaces" in _native.HOST_API
    for m in ("interface_points", "move_interfaces", "remap_colors"):
        assert callable(getattr(TransferContext, m))
