"""The two restatements of the group merge (tests/merge_ref.py) against each
other, and the properties of a merge that follow from its definition without
either (CPU only):

  - merge_par (array operations, the statement of include/parmmg_hip.h) equals
    merge_seq (the reference's loop, transcribed) in every array, on the six
    fixtures of contig_ref.MESH_CASES split by split_ref.split_seq, with and
    without old communicator positions, with nnode0 / nface0 of 0 and of 100;
  - the round trip: merge(split(mesh)) is the mesh again, up to the two
    permutations the calls return (old_tet o src_tet, old_pt o src_pt), and
    the merged mesh conforms;
  - the signs of the two intvalues arrays;
  - hand-written fixtures;
  - the symbols, and the host-built tables under ASan + UBSan."""
import functools
import os
import subprocess

import numpy as np
import pytest

import contig_ref as R
import merge_ref as M
import snapshot_ref
import split_ref as S

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@functools.lru_cache(maxsize=None)
def case(name, old, base):
    """(mesh, split, merge_seq, merge_par); base: what nnode0 / nface0 start from beside the old positions"""
    g = R.mesh_case(*name)
    kw = dict(nnode0=base, nface0=base)
    if old:
        node_pos, face_old, nnode0, nface0 = S.old_positions(g["tetv"], g["adja"], 7)
        kw = dict(node_pos=node_pos, face_old=face_old, nnode0=nnode0 + base, nface0=nface0 + base)
    sp = S.split_seq(g["tetv"], g["adja"], g["part"], g["ncolor"], g["np"], **kw)
    color = 10 + 3 * np.arange(g["ncolor"])
    return g, kw, sp, M.merge_seq(sp, color=color), M.merge_par(sp, color=color)


CASES = [(n, o, b) for n in R.MESH_CASES for o in (False, True) for b in (0, 100)]


@pytest.mark.parametrize("name,old,base", CASES, ids=str)
def test_par_equals_seq(name, old, base):
    g, kw, sp, seq, par = case(name, old, base)
    M.assert_same(par, seq)
    print(name, old, base, seq["np"], seq["ne"], int((seq["node_val"] != 0).sum()), int((seq["face_val"] != 0).sum()))


@pytest.mark.parametrize("name,old,base", CASES, ids=str)
def test_round_trip(name, old, base):
    """independent of both restatements' definitions: only the maps and the original mesh are used"""
    g, kw, sp, seq, _ = case(name, old, base)
    assert (seq["np"], seq["ne"]) == (g["np"], 6000)
    tet = sp["old_tet"][seq["src_tet"] - 1]  # the original tetra behind every merged tetra
    pnt = sp["old_pt"][seq["src_pt"] - 1]  # the original vertex behind every merged point
    assert sorted(tet.tolist()) == list(range(1, 6001))
    assert sorted(pnt.tolist()) == list(range(1, g["np"] + 1))
    np.testing.assert_array_equal(pnt[seq["tetv_out"] - 1], g["tetv"][tet - 1])
    # new_pt / new_tet are the inverse maps
    np.testing.assert_array_equal(seq["new_tet"][seq["src_tet"] - 1], np.arange(1, 6001))
    np.testing.assert_array_equal(pnt[seq["new_pt"] - 1], sp["old_pt"])
    # the merged mesh conforms: its adjacency is the original's, renamed
    adja, nonmanifold = snapshot_ref.adjacency(seq["tetv_out"])
    assert not nonmanifold
    merged_of = np.empty(6001, np.int64)
    merged_of[tet] = np.arange(1, 6001)
    a = g["adja"][tet - 1].astype(np.int64)
    np.testing.assert_array_equal(adja, np.where(a != 0, 4 * merged_of[a // 4] + a % 4, 0))
    # the marks: the colour of the group every merged tetra came from
    np.testing.assert_array_equal(seq["mark_out"], 10 + 3 * g["part"][tet - 1])


@pytest.mark.parametrize("name,old,base", CASES, ids=str)
def test_signs(name, old, base):
    g, kw, sp, seq, _ = case(name, old, base)
    te, pt, fa, no = S.segments(sp)
    pnt = sp["old_pt"][seq["src_pt"] - 1]
    vertex, holders = {}, {}
    for grp in range(g["ncolor"]):
        old_pt = sp["old_pt"][pt[grp]:pt[grp + 1]]
        for i1, i2 in zip(sp["node_idx1"][no[grp]:no[grp + 1]].tolist(), sp["node_idx2"][no[grp]:no[grp + 1]].tolist()):
            assert vertex.setdefault(i2, int(old_pt[i1 - 1])) == int(old_pt[i1 - 1])
            holders.setdefault(i2, set()).add(grp)
    val = seq["node_val"]
    assert val.size == sp["nnode_end"] and set(np.nonzero(val)[0].tolist()) == set(vertex)
    seen = set()
    for p, v in vertex.items():
        assert pnt[abs(val[p]) - 1] == v
        assert (val[p] > 0) == (len(holders[p]) % 2 == 1), (p, holders[p])
        seen.add(len(holders[p]))
    assert {1, 2, 3} <= seen or not old  # (old positions on the boundary: nodes of one group)
    assert {2, 3} <= seen  # two groups meet (negative), three groups meet (positive)
    # faces: negative exactly between two groups, positive on old parallel faces
    count = np.bincount(sp["face_idx2"], minlength=sp["nface_end"])
    fv = seq["face_val"]
    assert fv.size == sp["nface_end"]
    np.testing.assert_array_equal(fv < 0, count == 2)
    np.testing.assert_array_equal(fv > 0, count == 1)
    nface0 = kw["nface0"]
    assert (count[nface0:] == 2).all() and (count[:nface0] <= 1).all()
    assert (count[:nface0] == 1).any() == bool(old)
    # a value names the tetra, face and first vertex of the position's lowest entry, in the merged mesh
    for grp in range(g["ncolor"]):
        for i1, i2 in zip(sp["face_idx1"][fa[grp]:fa[grp + 1]].tolist(), sp["face_idx2"][fa[grp]:fa[grp + 1]].tolist()):
            if abs(fv[i2]) % 12 == i1 % 12 and seq["new_tet"][te[grp] + i1 // 12 - 1] == abs(fv[i2]) // 12:
                count[i2] = -1  # the entry whose value stands
    assert (count[np.nonzero(fv)[0]] == -1).all()


# ---------------------------------------------------------------- hand-written fixtures

def groups(*gs, nnode, nface):
    """split_ref's layout from per-group (tetv, node entries [(index1, index2)], face entries)"""
    z = lambda rows, w: np.array(rows, np.int32).reshape(-1, w)
    count = [(len(t), max([max(r) for r in t], default=0), len(f), len(n)) for t, n, f in gs]
    nodes = z([e for _, n, _ in gs for e in n], 2)
    faces = z([e for _, _, f in gs for e in f], 2)
    return dict(count=np.array(count, np.int32), tetv_out=z([r for t, _, _ in gs for r in t], 4),
                node_idx1=nodes[:, 0].copy(), node_idx2=nodes[:, 1].copy(), face_idx1=faces[:, 0].copy(),
                face_idx2=faces[:, 1].copy(), nnode_end=nnode, nface_end=nface)


def two_tetra():
    """DESIGN §12's fixture as the split leaves it (tests/test_gpu_split.py::test_two_tetra_two_groups): tetra
    (1, 2, 3, 4) and (3, 2, 5, 4) in two groups, nface0 = 10, nnode0 = 100"""
    sp = groups(([[1, 2, 3, 4]], [(2, 101), (3, 102), (4, 103)], [(12, 10)]),
                ([[1, 2, 3, 4]], [(1, 102), (2, 101), (4, 103)], [(19, 10)]), nnode=106, nface=11)
    node_val = np.zeros(106, np.int32)
    node_val[101:104] = [-2, -3, -4]  # two holders each
    face_val = np.zeros(11, np.int32)
    face_val[10] = -12  # group 0's index1, negated by group 1's entry
    want = dict(np=5, ne=2, new_pt=[1, 2, 3, 4, 3, 2, 5, 4], new_tet=[1, 2], src_pt=[1, 2, 3, 4, 7], src_tet=[1, 2],
                tetv_out=[[1, 2, 3, 4], [3, 2, 5, 4]], node_val=node_val, face_val=face_val, mark_out=[7, 9])
    return sp, [7, 9], want


def interface_tetra_last():
    """group 1's interface tetra are 3, then 2: the first-entry order is not the id order; its point 5 meets group
    0's point 2, its point 6 gets a new point before the unlisted ones"""
    sp = groups(([[1, 2, 3, 4]], [(2, 0)], [(12, 0)]),
                ([[1, 2, 3, 4], [2, 3, 4, 5], [3, 4, 5, 6]], [(5, 0), (6, 1)],
                 [(12 * 3 + 3 * 1 + 0, 0), (12 * 2 + 3 * 0 + 2, 1), (12 * 3 + 3 * 2 + 1, 2)]), nnode=3, nface=3)
    want = dict(np=9, ne=4, new_pt=[1, 2, 3, 4, 6, 7, 8, 9, 2, 5], new_tet=[1, 4, 3, 2], src_pt=[1, 2, 3, 4, 10, 5, 6, 7, 8],
                src_tet=[1, 4, 3, 2], tetv_out=[[1, 2, 3, 4], [8, 9, 2, 5], [7, 8, 9, 2], [6, 7, 8, 9]],
                node_val=[-2, 5, 0], face_val=[-12, 12 * 3 + 2, 12 * 2 + 7], mark_out=[4, 2, 2, 2])
    return sp, [4, 2], want


def point_listed_twice():
    """group 1 lists its point 2 at positions 0 and 1: the second entry is ignored and position 1 stays 0"""
    sp = groups(([[1, 2, 3, 4]], [], []), ([[1, 2, 3, 4]], [(2, 0), (2, 1), (3, 2)], []), nnode=3, nface=0)
    want = dict(np=8, ne=2, new_pt=[1, 2, 3, 4, 7, 5, 6, 8], new_tet=[1, 2], src_pt=[1, 2, 3, 4, 6, 7, 5, 8],
                src_tet=[1, 2], tetv_out=[[1, 2, 3, 4], [7, 5, 6, 8]], node_val=[5, 0, 6], face_val=[])
    return sp, None, want


def three_groups_at_a_node():
    """one node held by three groups (positive), one by two (negative), one by groups 1 and 2 only (a new point,
    negative)"""
    sp = groups(([[1, 2, 3, 4]], [(1, 0), (2, 1)], []), ([[1, 2, 3, 4]], [(1, 0), (3, 2)], []),
                ([[1, 2, 3, 4]], [(4, 0), (1, 1), (2, 2)], []), nnode=4, nface=0)
    # created: group 1's point 3 (5); unlisted: group 1's 2 and 4 (6, 7), then group 2's 3 (8)
    want = dict(np=8, ne=3, new_pt=[1, 2, 3, 4, 1, 6, 5, 7, 2, 5, 8, 1], new_tet=[1, 2, 3],
                src_pt=[1, 2, 3, 4, 7, 6, 8, 11], src_tet=[1, 2, 3],
                tetv_out=[[1, 2, 3, 4], [1, 6, 5, 7], [2, 5, 8, 1]], node_val=[1, -2, -5, 0], face_val=[])
    return sp, None, want


HAND = dict(two_tetra=two_tetra, interface_tetra_last=interface_tetra_last, point_listed_twice=point_listed_twice,
            three_groups_at_a_node=three_groups_at_a_node)


@pytest.mark.parametrize("which", sorted(HAND))
@pytest.mark.parametrize("ref", [M.merge_seq, M.merge_par], ids=["seq", "par"])
def test_hand_written(which, ref):
    sp, color, want = HAND[which]()
    got = ref(sp, color=color)
    assert (got["np"], got["ne"]) == (want["np"], want["ne"])
    for k in M.KEYS + (("mark_out",) if color is not None else ()):
        np.testing.assert_array_equal(got[k].reshape(-1), np.array(want[k], np.int32).reshape(-1), err_msg=k)


def test_preconditions_are_asserted():
    sp, _, _ = point_listed_twice()
    sp["node_idx1"][1] = 3  # position 1 ... and position 2 name point 3; make position 2 name two points
    sp["node_idx2"][1] = 2
    sp["node_idx1"][2] = 4
    for ref in (M.merge_seq, M.merge_par):
        with pytest.raises(AssertionError, match="names two points"):
            ref(sp)
    sp, _, _ = interface_tetra_last()
    sp["face_idx2"][2] = 0
    for ref in (M.merge_seq, M.merge_par):
        with pytest.raises(AssertionError, match="appears twice"):
            ref(sp)


# ---------------------------------------------------------------- the symbols, the host-built tables

def test_symbols():
    """the tables, the headers and the two libraries name the calls (fails without the feature)"""
    import ctypes

    from parmmg_amd import _native, build
    from parmmg_amd.transfer import TransferContext

    hip = ("pmmg_hip_merge_groups", "pmmg_hip_gather_rows_i32")
    host = ("pmmg_merge_grps", "pmmg_merge_result_free")
    header = open(os.path.join(ROOT, "include", "parmmg_hip.h")).read()
    host_header = open(os.path.join(ROOT, "parmmg_amd", "csrc", "pmmg_host.h")).read()

    def exports(so):
        out = subprocess.run(["nm", "-D", "--defined-only", so], stdout=subprocess.PIPE, text=True, check=True).stdout
        return {line.split()[-1] for line in out.splitlines() if line.strip()}

    for name in hip:
        assert name in _native.HIP_API and name in header and name in exports(build.HIP_SO)
    for name in host:
        assert name in _native.HOST_API and name in host_header and name in exports(build.HOST_SO)
    assert "pmmg_merge_result" in host_header
    assert ctypes.sizeof(_native.HostMergeResult) == 8 + 12 * 8  # two ints, nine pointers, met_size padded, two pointers
    for method in ("merge_groups", "gather_rows_i32", "merged_from_groups"):
        assert hasattr(TransferContext, method)
    assert _native.ABI_VERSION == 6 and "#define PMMG_HIP_ABI_VERSION 6" in header


def test_tables_under_sanitizers(tmp_path):
    """the host-built offset tables of pmmg_hip_merge_groups (csrc/pmmg_merge_tables.hpp) driven by the stand-alone
    tests/c/test_merge_tables.cpp, built with ASan + UBSan as tests/test_contig_ref_host.py builds its program"""
    import shutil

    cxx = shutil.which("g++") or shutil.which("clang++")
    if cxx is None:
        pytest.skip("no C++ compiler found")
    flags = ["-fsanitize=address,undefined", "-fno-omit-frame-pointer", "-fno-sanitize-recover=all"]
    probe_c, probe = tmp_path / "probe.cpp", tmp_path / "probe"
    probe_c.write_text("int main() { return 0; }\n")
    pr = subprocess.run([cxx] + flags + ["-o", str(probe), str(probe_c)], stdout=subprocess.PIPE,
                        stderr=subprocess.STDOUT, text=True)
    if pr.returncode != 0 or subprocess.run([str(probe)]).returncode != 0:
        pytest.skip("sanitizer runtime not available: " + pr.stdout[-200:])
    exe = tmp_path / "test_merge_tables"
    cmd = [cxx, "-O1", "-g", "-std=c++17", "-Wall", "-Wextra"] + flags + [
        f"-I{os.path.join(ROOT, 'parmmg_amd', 'csrc')}", f"-I{os.path.join(ROOT, 'include')}", "-o", str(exe),
        os.path.join(ROOT, "tests", "c", "test_merge_tables.cpp")]
    p = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert p.returncode == 0, p.stdout
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:halt_on_error=1")
    r = subprocess.run([str(exe)], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=120, env=env)
    assert r.returncode == 0, r.stdout[-3000:]
    assert "0 failed" in r.stdout
