"""The METIS element graph of a group, PMMG_graph_meshElts2metis (reference
src/metis_pmmg.c:746-823): the numpy restatement the device tests compare
with, its own invariants, the condition on the fixture that makes an exact
comparison of the truncated weights legitimate, and the symbols (CPU only).

Fixture: the jittered cube lattice n = 10 (6000 tetra, 22,800 graph entries)
with the synthetic iso and aniso metrics.  adjwgt = max((int)w, 1) truncates a
double the device holds to 1e-13 relative (tests/test_wgt.py), so the device
and the oracle can only disagree on an entry whose w lies within 1e-13
relative of an integer.  test_fixture_keeps_weights_off_integers asserts that
no uncapped oracle weight comes closer than 1e-11: a changed generator fails
there, on the CPU, and not in the exact comparisons on the GPU.  (At n = 6
every iso weight is capped at PMMG_WGTVAL_HUGEINT: that size tests nothing.)"""
import functools
import os
import subprocess

import numpy as np
import pytest

from oracle import oracle as O
from parmmg_amd import build, synth

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HUGE = 1.0e6  # PMMG_WGTVAL_HUGEINT
KINDS = ("iso", "aniso", "nomet", "noweights")


@functools.lru_cache(maxsize=None)
def fixture():
    """(mesh, {kind: metric or None}); shared by the tests, never modified"""
    bg = synth.lattice(synth.CUBE, 10, jitter=0.15, seed=3)
    mets = {"iso": synth.solution(synth.F_ISO, bg.xyz), "aniso": synth.solution(synth.F_ANI, bg.xyz), "nomet": None,
            "noweights": None}
    for a in (bg.xyz, bg.tetv, bg.adja, mets["iso"], mets["aniso"]):
        a.setflags(write=False)
    return bg, mets


@functools.lru_cache(maxsize=None)
def face_weights(kind):
    """the oracle's PMMG_computeWgt of every interior face of the fixture, [ne, 4] (NaN on boundary faces)"""
    bg, mets = fixture()
    w = np.full((bg.ne, 4), np.nan)
    for k in range(bg.ne):
        for f in range(4):
            if bg.adja[k, f]:
                w[k, f] = O.face_wgt(bg.xyz, bg.tetv[k], f, mets[kind])
    w.setflags(write=False)
    return w


def graph_ref(tetv, adja, kind, rows=None):
    """The loop of src/metis_pmmg.c:766-820 over adja rows in (tetra, face)
    order: (xadj, adjncy, adjwgt | None).  An unused tetra (v[0] <= 0) is an
    empty row.  The weight of face (k, f) is max(int(O.face_wgt(...)), 1) of
    the fixture's tetra rows[k] (default k): a cut of the fixture keeps its
    tetra, so the table face_weights() serves every variant."""
    ne = adja.shape[0]
    w = None if kind == "noweights" else face_weights(kind)
    xadj, adjncy, adjwgt = np.zeros(ne + 1, np.int32), [], []
    for k in range(ne):
        if tetv[k, 0] > 0:
            for f in range(4):
                if adja[k, f]:
                    adjncy.append(adja[k, f] // 4 - 1)
                    if w is not None:
                        adjwgt.append(max(int(w[k if rows is None else rows[k], f]), 1))
        xadj[k + 1] = len(adjncy)
    return xadj, np.array(adjncy, np.int32), (None if w is None else np.array(adjwgt, np.int32))


def cut(adja, keep):
    """adja with every link from or to a tetra outside the boolean mask keep[ne] set to 0"""
    a = np.array(adja)
    nb = a // 4 - 1
    a[(a != 0) & ~keep[np.where(a != 0, nb, 0)]] = 0
    a[~keep] = 0
    return a


@pytest.mark.parametrize("kind", ["iso", "aniso"])
def test_fixture_keeps_weights_off_integers(kind):
    bg, _ = fixture()
    w = face_weights(kind)[bg.adja != 0]
    assert w.size == 22800 and bg.ne == 6000
    assert np.isfinite(w).all() and (w > 0).all() and (w <= HUGE).all()
    free = w[w < HUGE]
    assert free.size > 5000  # (the size must test something: at n = 6 every iso weight is capped)
    dist = np.abs(free - np.rint(free)) / free
    print(kind, "range", w.min(), w.max(), "capped", int((w == HUGE).sum()), "closest to an integer", dist.min())
    assert dist.min() >= 1e-11


def test_fixture_weights_are_symmetric():
    """both tetra of a face measure the same three edges: no asymmetric pair after truncation"""
    bg, _ = fixture()
    for kind in ("iso", "aniso"):
        w = np.trunc(face_weights(kind))
        k, f = np.nonzero(bg.adja)
        nb, nf = bg.adja[k, f] // 4 - 1, bg.adja[k, f] % 4
        np.testing.assert_array_equal(w[k, f], w[nb, nf])


@pytest.mark.parametrize("kind", KINDS)
def test_restatement_invariants(kind):
    bg, _ = fixture()
    xadj, adjncy, adjwgt = graph_ref(bg.tetv, bg.adja, kind)
    assert xadj[0] == 0 and xadj[-1] == np.count_nonzero(bg.adja) == adjncy.size
    assert (np.diff(xadj) >= 0).all() and (np.diff(xadj) <= 4).all()
    assert adjncy.min() >= 0 and adjncy.max() < bg.ne
    edges = set()
    for k in range(bg.ne):
        for e in range(xadj[k], xadj[k + 1]):
            edges.add((k, int(adjncy[e])))
    assert all((b, a) in edges for a, b in edges)  # every entry's reverse entry exists
    if kind == "noweights":
        assert adjwgt is None
    else:
        assert adjwgt.size == adjncy.size and (adjwgt >= 1).all() and (adjwgt <= int(HUGE)).all()
        if kind == "nomet":
            assert (adjwgt == int(HUGE)).all()


def test_restatement_of_a_cut_mesh():
    """the variants the device tests use: a prefix of the mesh, a band of empty rows, an unused row"""
    bg, _ = fixture()
    keep = np.arange(bg.ne) < 65
    a = cut(bg.adja, keep)[:65]
    assert ((a // 4) <= 65).all()
    xadj, adjncy, _ = graph_ref(bg.tetv[:65], a, "iso")
    assert xadj[-1] == np.count_nonzero(a) and adjncy.max() < 65
    keep = np.ones(bg.ne, bool)
    keep[256:768] = False
    a = cut(bg.adja, keep)
    xadj, _, _ = graph_ref(bg.tetv, a, "iso")
    nb = a[a != 0] // 4 - 1
    assert (np.diff(xadj)[256:768] == 0).all() and not ((nb >= 256) & (nb < 768)).any()
    assert graph_ref(bg.tetv[:1], cut(bg.adja, np.arange(bg.ne) < 1)[:1], "iso")[0].tolist() == [0, 0]


def test_symbols():
    """the table, the header and the two libraries name the call (fails without the feature)"""
    from parmmg_amd import _native

    assert "pmmg_hip_metis_graph" in _native.HIP_API
    assert "pmmg_graph_mesh_elts2metis" in _native.HOST_API
    assert "pmmg_hip_metis_graph" in open(os.path.join(ROOT, "include", "parmmg_hip.h")).read()
    assert "pmmg_graph_mesh_elts2metis" in open(os.path.join(ROOT, "parmmg_amd", "csrc", "pmmg_host.h")).read()

    def exports(so):
        out = subprocess.run(["nm", "-D", "--defined-only", so], stdout=subprocess.PIPE, text=True, check=True).stdout
        return {line.split()[-1] for line in out.splitlines() if line.strip()}

    assert "pmmg_hip_metis_graph" in exports(build.HIP_SO)
    assert "pmmg_graph_mesh_elts2metis" in exports(build.HOST_SO)
