"""The two restatements of the group split (tests/split_ref.py) against each
other, and the properties of a split that follow from its definition without
either (CPU only):

  - split_par (array operations, the statement of include/parmmg_hip.h) equals
    split_seq (the reference's loop, transcribed) in every array, on the six
    fixtures of contig_ref.MESH_CASES, with and without old communicator
    positions;
  - every group is a conforming mesh: the adjacency built from its tetv_out by
    the snapshot's definition is its adja_out;
  - every new face position occurs exactly twice over all groups, and the two
    iplocs name the same old vertex; a node position belongs to one old vertex;
  - the counts add up and old_tet is a permutation;
  - case "c" puts nearly every vertex in all three groups."""
import functools

import numpy as np
import pytest

import contig_ref as R
import snapshot_ref
import split_ref as S


@functools.lru_cache(maxsize=None)
def both(name, old):
    g = R.mesh_case(*name)
    kw = {}
    if old:
        node_pos, face_old, nnode0, nface0 = S.old_positions(g["tetv"], g["adja"], 7)
        kw = dict(node_pos=node_pos, face_old=face_old, nnode0=nnode0, nface0=nface0)
    args = (g["tetv"], g["adja"], g["part"], g["ncolor"], g["np"])
    return g, kw, S.split_seq(*args, **kw), S.split_par(*args, **kw)


CASES = [(n, o) for n in R.MESH_CASES for o in (False, True)]


@pytest.mark.parametrize("name,old", CASES, ids=str)
def test_par_equals_seq(name, old):
    g, kw, seq, par = both(name, old)
    S.assert_same(par, seq)
    print(name, old, seq["count"].tolist(), seq["nnode_end"], seq["nface_end"])


@pytest.mark.parametrize("name,old", CASES, ids=str)
def test_every_group_is_a_conforming_mesh(name, old):
    g, kw, seq, _ = both(name, old)
    te, pt, _, _ = S.segments(seq)
    assert te[-1] == 6000 and sorted(seq["old_tet"].tolist()) == list(range(1, 6001))
    np.testing.assert_array_equal(seq["new_tet"][seq["old_tet"] - 1],
                                  np.concatenate([np.arange(1, n + 1) for n in seq["count"][:, 0]]))
    for grp in range(g["ncolor"]):
        tv = seq["tetv_out"][te[grp]:te[grp + 1]]
        adja, nonmanifold = snapshot_ref.adjacency(tv)
        assert not nonmanifold
        np.testing.assert_array_equal(adja, seq["adja_out"][te[grp]:te[grp + 1]])
        # the points: ids 1 .. np in order of first use, and the old vertices behind them
        old_pt = seq["old_pt"][pt[grp]:pt[grp + 1]]
        flat = tv.reshape(-1)
        _, first = np.unique(flat, return_index=True)
        assert flat[np.sort(first)].tolist() == list(range(1, old_pt.size + 1))
        np.testing.assert_array_equal(old_pt[tv - 1], g["tetv"][seq["old_tet"][te[grp]:te[grp + 1]] - 1])


@pytest.mark.parametrize("name,old", CASES, ids=str)
def test_positions(name, old):
    g, kw, seq, _ = both(name, old)
    te, pt, fa, no = S.segments(seq)
    nface0 = kw.get("nface0", 0)
    seen = {}
    for grp in range(g["ncolor"]):
        tv_old = g["tetv"][seq["old_tet"][te[grp]:te[grp + 1]] - 1]
        for i1, i2 in zip(seq["face_idx1"][fa[grp]:fa[grp + 1]].tolist(), seq["face_idx2"][fa[grp]:fa[grp + 1]].tolist()):
            t, f, iploc = i1 // 12, (i1 % 12) // 3, i1 % 3
            seen.setdefault(i2, []).append(int(tv_old[t - 1, S.IDIR[f][iploc]]))
    new = {p: v for p, v in seen.items() if p >= nface0}
    assert sorted(new) == list(range(nface0, seq["nface_end"]))
    assert all(len(v) == 2 and v[0] == v[1] for v in new.values())
    assert all(len(v) == 1 for p, v in seen.items() if p < nface0)
    # a node position belongs to one old vertex, and a vertex has one position
    by_pos, by_vert = {}, {}
    for grp in range(g["ncolor"]):
        old_pt = seq["old_pt"][pt[grp]:pt[grp + 1]]
        for i1, i2 in zip(seq["node_idx1"][no[grp]:no[grp + 1]].tolist(), seq["node_idx2"][no[grp]:no[grp + 1]].tolist()):
            by_pos.setdefault(i2, set()).add(int(old_pt[i1 - 1]))
            by_vert.setdefault(int(old_pt[i1 - 1]), set()).add(i2)
    assert all(len(v) == 1 for v in by_pos.values()) and all(len(p) == 1 for p in by_vert.values())
    # nitem counts entries: the positions have gaps
    assert seq["nnode_end"] == kw.get("nnode0", 0) + int(seq["count"][:, 3].sum())
    assert max(by_pos) <= seq["nnode_end"] and len(by_pos) < seq["nnode_end"]


def test_case_c_is_the_worst_case_of_shared_vertices():
    _, _, seq, _ = both(("c", False), False)
    assert seq["count"][:, 1].tolist() == [1309, 1308, 1312]
    assert int(seq["count"][:, 2].sum()) == 15128 == 2 * seq["nface_end"]  # interface faces, seen from both sides
