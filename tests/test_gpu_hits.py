"""Every hit kind of the reference's locate functions produced on the GPU
and checked against the oracle (runs on the MI355X).

  2 VOL_EXHAUST   walk stopped (test-only PMMG_HIP_MAXSTEP=1), accepting
                  brute force: the lowest-index accepting tetra
                  (PMMG_locatePoint_exhaustTetra, locate_pmmg.c:737-770)
  3 VOL_CLOSEST   volume point outside the background: closest tetra
  7 BDY_WEDGE     surface point beyond a cube edge, within hausd of it
                  (PMMG_locatePointInWedge, locate_pmmg.c:286-334)
  8 BDY_CONE      surface point beyond a cube corner, within hausd of it
                  (PMMG_locatePointInCone, locate_pmmg.c:209-270)
  9 BDY_EXHAUST   surface walk stopped (PMMG_HIP_MAXSTEP=1): the
                  lowest-index accepting tria (locate_pmmg.c:477-515)
 11 BDY_CLOSEST   surface point beyond hausd of every tria
 10 BDY_STALE     the reference re-evaluates the last scanned tria with the
                  closest tria's normal after a failed exhaustive search
                  (locate_pmmg.c:505-512): reached by a constructed fixture
                  (tests/parity.py::stale_case, r06; random points around the
                  lattices never reach it: the closest tria's normal never
                  accepts where the last tria's own test failed).
Each test compares with tests/parity.py::check (acceptance for the hit kind,
values of the reference interpolator, class (i) identity against the
oracle's run)."""
import numpy as np
import pytest

from oracle import oracle as O
from parity import assert_stats_match, check, make_case, run_gpu
from parmmg_amd import synth


def _codes(gpu):
    return np.bincount(gpu["hit"].astype(np.int32) & 15, minlength=12)


def _with_points(case, xyz):
    import dataclasses
    case = dict(case)
    case["new"] = dataclasses.replace(case["new"], xyz=np.ascontiguousarray(xyz))
    vis = synth.visit_order(case["new"])
    case["ref"] = O.run(case["B"], case["new"].xyz, case["pclass"], vis, O.MODE_FRESH)
    return case


@pytest.mark.gpu
def test_forced_exhaustive_hits(monkeypatch):
    """PMMG_HIP_MAXSTEP=1 (test-only): walks stop after one step, so the
    exhaustive kernels run for most points: codes 2 and 9, each the
    lowest-index accepting element."""
    monkeypatch.setenv("PMMG_HIP_MAXSTEP", "1")  # read by pmmg_hip_create
    case = make_case(kind=synth.CUBE, n_old=5, n_new=6)
    gpu = run_gpu(case, tet8=True)
    rep = check(case, gpu)
    c = _codes(gpu)
    print(rep, c)
    assert c[2] > 0 and c[9] > 0
    assert rep["class_i"] == rep["class_i_same"]
    assert_stats_match(gpu["stats"], case["pclass"], gpu["hit"], maxstep=1)


@pytest.mark.gpu
@pytest.mark.parametrize("packed", [False, True])
def test_cone_and_wedge_hits(packed):
    """Surface points pushed beyond the cube's corners (cone, code 8) and
    edges (wedge, code 7) by less than hausd; values from the corner vertex
    (copyMetrics) / the edge (interp2bar)."""
    case = make_case(kind=synth.CUBE, n_old=6, n_new=7, fields=(synth.F_SCALAR, synth.F_VECTOR, synth.F_TENSOR),
                     with_ref=False)
    x = case["new"].xyz.copy()
    corner = np.all(np.isclose(x, 0) | np.isclose(x, 1), axis=1)
    on_edge = (np.sum(np.isclose(x, 0) | np.isclose(x, 1), axis=1) == 2)
    for i in np.nonzero(corner)[0]:
        x[i] += 0.003 * np.where(x[i] > 0.5, 1.0, -1.0)
    for i in np.nonzero(on_edge)[0]:
        d = np.where(np.isclose(x[i], 1), 1.0, np.where(np.isclose(x[i], 0), -1.0, 0.0))
        x[i] += 0.004 * d
    case = _with_points(case, x)
    gpu = run_gpu(case, tet8=True, packed=packed)
    rep = check(case, gpu)
    c = _codes(gpu)
    print(rep, c, "oracle:", np.bincount(case["ref"]["hit"], minlength=12))
    assert c[8] == int(corner.sum()) and c[7] > 0
    assert ((gpu["hit"][corner] & 15) == 8).all()


@pytest.mark.gpu
def test_cone_fan_scan_equals_rotation(monkeypatch):
    """The cone test walks the vertex's tria fan through adjt and falls back
    to scanning every tria (the node->tria list) when the fan is open,
    non-manifold or longer than kFanMax.  Test-only PMMG_HIP_FANMAX=1 sends
    every cone test through the scan: same hits, same elements, bit-identical
    rows as the rotation."""
    case = make_case(kind=synth.CUBE, n_old=6, n_new=7, fields=(synth.F_SCALAR, synth.F_VECTOR), with_ref=False)
    x = case["new"].xyz.copy()
    corner = np.all(np.isclose(x, 0) | np.isclose(x, 1), axis=1)
    for i in np.nonzero(corner)[0]:
        x[i] += 0.003 * np.where(x[i] > 0.5, 1.0, -1.0)
    case = _with_points(case, x)
    base = run_gpu(case, tet8=True)
    monkeypatch.setenv("PMMG_HIP_FANMAX", "1")  # read by pmmg_hip_create
    scan = run_gpu(case, tet8=True)
    assert _codes(base)[8] == int(corner.sum())
    np.testing.assert_array_equal(scan["hit"], base["hit"])
    np.testing.assert_array_equal(scan["elem"], base["elem"])
    np.testing.assert_array_equal(scan["met"], base["met"])
    for a, b in zip(scan["fields"], base["fields"]):
        np.testing.assert_array_equal(a, b)
    assert check(case, scan)["class_i"] >= 0


@pytest.mark.gpu
def test_closest_hits():
    """Volume points outside the background (code 3: closest tetra) and
    surface points beyond hausd of every tria (code 11: closest tria)."""
    case = make_case(kind=synth.CUBE, n_old=5, n_new=6, with_ref=False)
    x = case["new"].xyz.copy()
    rng = np.random.default_rng(5)
    vol = np.nonzero(case["pclass"] == 1)[0]
    bdy = np.nonzero(case["pclass"] == 2)[0]
    pv = rng.choice(vol, 12, replace=False)
    pb = rng.choice(bdy, 12, replace=False)
    x[pv, 0] = 1.0 + rng.uniform(0.01, 0.3, 12)
    for i in pb:  # outward along the nearest face normal, beyond hausd
        a = int(np.argmin(np.minimum(x[i], 1 - x[i])))
        x[i, a] += -0.05 if x[i, a] < 0.5 else 0.05
    case = _with_points(case, x)
    gpu = run_gpu(case, tet8=True)
    rep = check(case, gpu)
    c = _codes(gpu)
    print(rep, c)
    assert c[3] > 0 and c[11] > 0
    assert ((gpu["hit"][pb] & 15) == (case["ref"]["hit"][pb] & 15)).all()


@pytest.mark.gpu
@pytest.mark.parametrize("kind,n_old,n_new", [(synth.CUBE, 8, 9), (synth.SHELL, 8, 12)])
def test_surface_walks_from_one_far_seed(monkeypatch, kind, n_old, n_new):
    """PMMG_HIP_SRFG=1 (test-only): one surface seed cell, so every surface
    walk starts at the same tria and crosses the surface; on the shell the
    inner sphere cannot be reached from the outer one (or the reverse): those
    walks run through the 4-entry visited history until maxstep and fall to
    the exhaustive search.  The cost of that path is known and the results
    still meet the contract (tests/parity.py)."""
    monkeypatch.setenv("PMMG_HIP_SRFG", "1")
    monkeypatch.setenv("PMMG_HIP_MAXSTEP", "256")
    case = make_case(kind=kind, n_old=n_old, n_new=n_new)
    gpu = run_gpu(case, tet8=True)
    rep = check(case, gpu)
    st = gpu["stats"]
    c = _codes(gpu)
    print(kind, rep, c, {k: st[k] for k in ("nbdy", "nbdy_exhaust", "steps_total", "stepmax", "ms_bdy")})
    assert rep["n"] == int((case["pclass"] != 0).sum())
    assert rep["class_i"] == rep["class_i_same"]
    assert st["stepmax"] > 10
    if kind == synth.SHELL:
        assert st["nbdy_exhaust"] > 0


def two_cubes_case():
    """Two 16-cell cubes far apart ([0,1]^3 and [10,11]^3) whose tetra 1 is
    unused (v = 0, its neighbours' adjacency cleared, as MMG leaves a deleted
    tetra), new points in both cubes, and one volume query at (0, 11, 0):
    no background tetra within 6 seed cells of it in either the uniform or
    the quantile-mapped seed grid.  Its walk starts from the lowest in-use
    tetra the seed grid sampled (never from the unused tetra 1), gets stuck
    on the cube's boundary, and ends in the exhaustive search: the closest
    tetra (code 3)."""
    import dataclasses
    a = synth.lattice(synth.CUBE, 16)
    off = a.np
    ne = a.ne
    xyz = np.vstack([a.xyz, a.xyz + 10.0])
    tetv = np.vstack([a.tetv, a.tetv + off]).astype(np.int32)
    adja = np.vstack([a.adja, np.where(a.adja > 0, a.adja + 4 * ne, 0)]).astype(np.int32)
    triv = np.vstack([a.triv, a.triv + off]).astype(np.int32)
    adjt = np.vstack([a.adjt, np.where(a.adjt > 0, a.adjt + 3 * a.nt, 0)]).astype(np.int32)
    tetv[0] = 0
    adja[0] = 0
    adja[(adja >> 2) == 1] = 0
    bg = dataclasses.replace(a, xyz=xyz, tetv=tetv, adja=adja, triv=triv, adjt=adjt,
                             isbdy=np.concatenate([a.isbdy, a.isbdy]))
    b = synth.lattice(synth.CUBE, 5, jitter=0.2, with_trias=False, with_tetra=False)
    far = np.array([[0.0, 11.0, 0.0]])
    nxyz = np.vstack([b.xyz, b.xyz + 10.0, far])
    isbdy = np.concatenate([b.isbdy, b.isbdy, [0]]).astype(np.uint8)
    new = dataclasses.replace(b, xyz=nxyz, isbdy=isbdy)
    pc = np.where(isbdy == 1, 2, 1).astype(np.uint8)
    met = synth.solution(synth.F_ANI, xyz)
    fs = [synth.solution(synth.F_SCALAR, xyz), synth.solution(synth.F_TENSOR, xyz)]
    B = O.Background(bg, met, fs, 0.01)
    # no oracle run: the reference's own walk cannot start on an unused tetra
    # 1 (src/locate_pmmg.c:795-811 spins to step > ne, then takes the
    # "closest" tetra 0); check() still verifies every point's acceptance and
    # values against the oracle's element tests, which skip unused tetra
    return dict(bg=bg, new=new, met=met, fields=fs, pclass=pc, B=B, hausd=0.01)


@pytest.mark.gpu
@pytest.mark.parametrize("mode", [dict(), dict(sort=True), dict(tet8=True)])
def test_unused_tetra_one_and_empty_seed_neighbourhood(mode):
    """The last-resort seed of a query with an empty seed neighbourhood is
    a sampled tetra in use, not tetra 1 (tetra 1 unused made the
    walk read vertex 0, before the start of the coordinate arrays)."""
    case = two_cubes_case()
    gpu = run_gpu(case, **mode)
    rep = check(case, gpu)
    st = gpu["stats"]
    print(rep, {k: st[k] for k in ("nvol", "nvol_noseed", "nvol_exhaust", "nvol_closest", "nvol_stuck")})
    assert rep["n"] == case["new"].np and rep["class_i"] == rep["class_i_same"]
    assert st["nvol_noseed"] >= 1
    assert (gpu["hit"][-1] & 15) == 3
    assert O.first_accepting_tetra(case["B"], case["new"].xyz[-1]) == 0


@pytest.mark.gpu
@pytest.mark.parametrize("tet8", [False, True])
def test_stale_reevaluation_hits(tet8):
    """Code 10 (BDY_STALE) on the constructed fixture of tests/parity.py::
    stale_case: every surface point's walk and exhaustive search fail, the
    closest tria (1) differs from the last (2), and the re-evaluation with
    tria 2's vertices and tria 1's normal accepts.  The module's hit codes,
    elements and values equal the oracle's faithful run bit for bit (and the
    numpy restatement of that arithmetic within 1e-13)."""
    from parity import stale_case

    case, exp = stale_case()
    n = case["new"].xyz.shape[0]
    ref = O.run(case["B"], case["new"].xyz, case["pclass"], np.arange(1, n + 1, dtype=np.int32), O.MODE_FAITHFUL)
    gpu = run_gpu(case, tet8=tet8)
    print(gpu["hit"], gpu["elem"], gpu["stats"])
    assert (gpu["hit"] & 15 == 10).all() and (gpu["elem"] == 1).all()
    assert gpu["stats"]["nbdy_stale"] == n
    assert np.array_equal(gpu["met"].view(np.uint64), ref["met"].view(np.uint64))
    assert np.array_equal(gpu["fields"][0].view(np.uint64), ref["fields"][0].view(np.uint64))
    assert np.allclose(gpu["met"], exp["met"], rtol=1e-13, atol=0)


@pytest.mark.gpu
def test_long_volume_walks_and_the_step_cap():
    """walks long enough to reach the step cap.  One volume seed
    cell (PMMG_HIP_TPC=4096 on ~10k tetra: every walk starts from the same
    tetra and crosses the cube, tens of steps); first with the default cap
    (nothing capped: every walk ends in an accepting tetra, class (i)
    identical to the oracle's walk), then with the cap at a third of the
    longest of those walks: the capped walks go to the exhaustive search,
    whose lowest accepting index may differ from the reference's walk only
    for points several tetra accept (class (ii)); the contract still holds."""
    case = make_case(kind=synth.CUBE, n_old=12, n_new=13)
    gpu = run_gpu(case, tet8=True, env={"PMMG_HIP_TPC": "4096"})
    rep = check(case, gpu)
    st = gpu["stats"]
    print(rep, {k: st[k] for k in ("stepmax", "nvol_limit", "nvol_exhaust", "steps_total")})
    assert st["stepmax"] > 12 and st["nvol_limit"] == 0 and st["nvol_exhaust"] == 0
    assert rep["class_i"] == rep["class_i_same"]
    # (a capped filter walk hands over to the exact walk, which has the same cap: a walk of L steps is cut
    # only when L > 2 cap)
    cap = max(2, int(st["stepmax"]) // 3)
    gpu2 = run_gpu(case, tet8=True, env={"PMMG_HIP_TPC": "4096", "PMMG_HIP_MAXSTEP": str(cap)})
    rep2 = check(case, gpu2)
    st2 = gpu2["stats"]
    print(cap, rep2, {k: st2[k] for k in ("stepmax", "nvol_limit", "nvol_exhaust")})
    assert st2["nvol_limit"] > 0 and st2["nvol_exhaust"] >= st2["nvol_limit"]
    assert rep2["class_i"] == rep2["class_i_same"]
