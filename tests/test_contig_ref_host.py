"""The restatement of the reference's contiguity code (tests/contig_ref.py)
against itself, and the conditions on the fixtures that make the device tests
of tests/test_gpu_contig.py mean what they say (CPU only).

  - the ascending sweeps of PMMG_check_part_contiguity leave flag = 1 + the
    rank of the subgroup among its colour's heads;
  - the statement of include/parmmg_hip.h (no flags) equals the reference's
    flagged loop under the module's choice of the neighbouring colour, on every
    fixture;
  - the module's choice (lowest (tetra, face)) equals the reference's (first
    in BFS order from the head) on every lattice-numbered fixture: the device
    test on those is a test against the reference; the two differ on a
    scrambled one;
  - the fixtures have what they are there for, computed from them."""
import os
import subprocess

import numpy as np
import pytest

import contig_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def case(name):
    """(adja, part as an array, ncolor, part as passed to the calls)"""
    g = R.mesh_case(*name) if isinstance(name, tuple) else R.graph_case(name)
    part = g["part"] if g["part"] is not None else np.zeros(g["adja"].shape[0], np.int32)
    return g["adja"], part, g["ncolor"], g["part"]


ALL = R.MESH_CASES + R.SMALL_GRAPHS + R.PATH_GRAPHS


@pytest.mark.parametrize("name", ALL, ids=str)
def test_sweeps_leave_the_rank_by_head(name):
    adja, part, ncolor, _ = case(name)
    head, flag, ncomp, table = R.subgroups(adja, part, ncolor)
    swept, sweeps = R.sweep_flags(adja, part, ncolor)
    print(name, "subgroups", ncomp.tolist(), "sweeps", sweeps)
    np.testing.assert_array_equal(swept, flag)
    # the table itself: ascending heads, sizes that add up, one head per subgroup
    assert (np.diff(table[:, 1]) > 0).all() and table[:, 2].sum() == adja.shape[0]
    assert (head[table[:, 1] - 1] == table[:, 1]).all() and ncomp.sum() == table.shape[0]
    for c in range(ncolor):
        assert flag[part == c].max(initial=0) == ncomp[c]


@pytest.mark.parametrize("name", ALL, ids=str)
def test_flag_free_statement_equals_the_flagged_loop(name):
    adja, part, ncolor, _ = case(name)
    flagged, free = R.fix_flagged(adja, part, ncolor, "lowest"), R.fix_free(adja, part, ncolor)
    assert int((flagged["part"] != free["part"]).sum()) == 0
    for k in ("nmoved", "nmerged", "nstuck"):
        assert flagged[k] == free[k], k


@pytest.mark.parametrize("cs", "abc")
def test_rules_agree_on_the_lattice_numbering(cs):
    adja, part, ncolor, _ = case((cs, False))
    low, bfs = R.fix_flagged(adja, part, ncolor, "lowest"), R.fix_flagged(adja, part, ncolor, "bfs")
    print(cs, "moved subgroups", low["nmerged"], "tetra", low["nmoved"])
    assert int((low["part"] != bfs["part"]).sum()) == 0 and low["nmerged"] == bfs["nmerged"] > 0
    assert R.subgroups(adja, low["part"], ncolor)[2].max() == 1


def test_rules_differ_on_a_scrambled_numbering():
    diff = {}
    for cs in "abc":
        adja, part, ncolor, _ = case((cs, True))
        low, bfs = R.fix_flagged(adja, part, ncolor, "lowest"), R.fix_flagged(adja, part, ncolor, "bfs")
        diff[cs] = int((low["part"] != bfs["part"]).sum())
        for r in (low, bfs):  # under both rules every colour ends as one subgroup
            assert R.subgroups(adja, r["part"], ncolor)[2].max() == 1
    print("tetra that differ between the rules:", diff)
    assert max(diff.values()) > 0


def test_fixture_conditions():
    moves = []
    for name in R.MESH_CASES:
        adja, part, ncolor, _ = case(name)
        ncomp = R.subgroups(adja, part, ncolor)[2]
        fix = R.fix_free(adja, part, ncolor)
        print(name, "subgroups per colour", ncomp.tolist(), "moved", fix["nmerged"], "tetra", fix["nmoved"])
        assert adja.shape[0] == 6000 and ncomp.max() >= 3 and ncomp.min() >= 1
        if name[0] == "c":
            assert ncomp.sum() > 2000
        moves += fix["moves"]
    assert any(to < c for c, to, _ in moves) and any(to > c for c, to, _ in moves)
    assert any(replaced for _, _, replaced in moves)
    # a scrambled numbering is one: the lattice's neighbours are close in number, these are not
    a0, a1 = R.mesh_case("a", False)["adja"], R.mesh_case("a", True)["adja"]
    gap = lambda a: np.abs(R.nbrs(a) - np.arange(a.shape[0])[:, None])[a != 0].mean()
    assert gap(a1) > 10 * gap(a0)


def test_small_graphs():
    adja, part, ncolor, _ = case("path7")
    good, wrong = R.fix_free(adja, part, ncolor), R.fix_oneshot(adja, part, ncolor)
    assert good["part"].tolist() == [0, 0, 0, 1, 1, 1, 1] and (good["nmerged"], good["nmoved"]) == (1, 1)
    assert wrong["part"].tolist() == [0, 0, 0, 0, 1, 1, 1]  # {4} moved into colour 0: two moves where one does
    assert R.subgroups(adja, good["part"], ncolor)[2].tolist() == [1, 1]

    adja, part, ncolor, _ = case("equal")
    fix = R.fix_free(adja, part, ncolor)
    assert fix["part"].tolist() == [0, 0, 1, 1, 1] and fix["moves"] == [(0, 1, False)]

    adja, part, ncolor, _ = case("stuck")
    fix = R.fix_free(adja, part, ncolor)
    assert (fix["part"] == part).all() and (fix["nmerged"], fix["nstuck"]) == (0, 1)
    assert R.subgroups(adja, part, ncolor)[3].tolist()[0] == [0, 1, 2, 0]  # main: no exit

    adja, part, ncolor, _ = case("stuck_later")
    fix = R.fix_free(adja, part, ncolor)
    # {7, 8, 9} is larger than the old main {1, 2} and not larger than {3, 4, 5}: with the old main it is stuck
    assert fix["nstuck"] == 2 and fix["part"].tolist() == [0, 0, 0, 0, 0, 0, 0, 0, 0, 1, 1, 1]
    assert fix["moves"] == [(0, 1, False), (1, 0, True)]

    adja, part, ncolor, _ = case("two_blocks")
    table = R.subgroups(adja, part, ncolor)[3]
    assert table.tolist() == [[0, 1, 3, 0], [1, 4, 4, 0]] and R.fix_free(adja, part, ncolor)["nmerged"] == 0

    adja, part, ncolor, _ = case("empty_colour")
    assert R.subgroups(adja, part, ncolor)[2].tolist() == [2, 0, 2]


@pytest.mark.parametrize("name", R.PATH_GRAPHS)
def test_scrambled_paths(name):
    adja, part, ncolor, given = case(name)
    n = adja.shape[0]
    assert ((adja != 0).sum(axis=1) <= 2).all() and (adja != 0).sum() == 2 * (n - 1)
    k, f = np.nonzero(adja)  # symmetric: the link names the face that points back
    assert (adja[adja[k, f] // 4 - 1, adja[k, f] % 4] // 4 - 1 == k).all()
    ncomp = R.subgroups(adja, part, ncolor)[2]
    bands = -(-n // 64)
    assert ncomp.tolist() == ([1] if given is None else [(bands + 1) // 2, bands // 2])


@pytest.mark.parametrize("name", R.TREE_GRAPHS)
def test_adversarial_trees(name):
    """the trees need more hooking rounds than ceil(log2 n) + 1, the bound one might take for the scheme's, and
    stay within the proven one; they are symmetric adjacencies of one subgroup"""
    adja, part, ncolor, _ = case(name)
    n = adja.shape[0]
    k, f = np.nonzero(adja)
    assert (adja[adja[k, f] // 4 - 1, adja[k, f] % 4] // 4 - 1 == k).all() and (adja != 0).sum() == 2 * (n - 1)
    assert R.subgroups(adja, None, 1)[3].tolist() == [[0, 1, n, 0]]
    rounds, labels = R.hook_rounds(adja)
    print(name, "rounds", rounds, "ceil(log2 n) + 1 =", int(np.ceil(np.log2(n))) + 1, "bound", R.round_bound(n))
    assert rounds == R.TREE_ROUNDS[name] and (labels == 0).all()
    assert int(np.ceil(np.log2(n))) + 1 < rounds <= R.round_bound(n)


@pytest.mark.parametrize("name", ALL + R.TREE_GRAPHS, ids=str)
def test_simulated_rounds_stay_within_the_bound(name):
    """the scheme, simulated round by round, labels every fixture by its subgroups' lowest tetra within the bound
    the device test holds the device to"""
    adja, part, ncolor, given = case(name)
    rounds, labels = R.hook_rounds(adja, given)
    print(name, "rounds", rounds, "bound", R.round_bound(adja.shape[0]))
    np.testing.assert_array_equal(labels + 1, R.subgroups(adja, given, ncolor)[0])
    assert rounds <= R.round_bound(adja.shape[0])
    if name == "scrambled65537_one":
        assert rounds == 11


def test_symbols():
    """the tables, the headers and the two libraries name the calls (fails without the feature)"""
    from parmmg_amd import _native, build
    from parmmg_amd.transfer import TransferContext

    hip = ("pmmg_hip_part_subgroups", "pmmg_hip_fix_contiguity")
    host = ("pmmg_check_part_contiguity", "pmmg_fix_contiguity_split")
    header = open(os.path.join(ROOT, "include", "parmmg_hip.h")).read()
    host_header = open(os.path.join(ROOT, "parmmg_amd", "csrc", "pmmg_host.h")).read()

    def exports(so):
        out = subprocess.run(["nm", "-D", "--defined-only", so], stdout=subprocess.PIPE, text=True, check=True).stdout
        return {line.split()[-1] for line in out.splitlines() if line.strip()}

    for name in hip:
        assert name in _native.HIP_API and name in header and name in exports(build.HIP_SO)
    for name in host:
        assert name in _native.HOST_API and name in host_header and name in exports(build.HOST_SO)
    assert "pmmg_hip_subgroup" in header
    import ctypes
    assert ctypes.sizeof(_native.HipSubgroup) == 16
    assert hasattr(TransferContext, "part_subgroups") and hasattr(TransferContext, "fix_contiguity")
    assert _native.ABI_VERSION == 6 and "#define PMMG_HIP_ABI_VERSION 6" in header


def test_decision_loop_under_sanitizers(tmp_path):
    """the host-side decision of pmmg_hip_fix_contiguity (csrc/pmmg_contig_decide.hpp) driven by the stand-alone
    tests/c/test_contig_decide.cpp, built with ASan + UBSan as tests/test_devbuf_host.py builds its program"""
    import shutil

    cxx = shutil.which("g++") or shutil.which("clang++")
    if cxx is None:
        pytest.skip("no C++ compiler found")
    exe = tmp_path / "test_contig_decide"
    cmd = [cxx, "-O1", "-g", "-std=c++17", "-Wall", "-Wextra", "-fsanitize=address,undefined",
           "-fno-omit-frame-pointer", "-fno-sanitize-recover=all", f"-I{os.path.join(ROOT, 'parmmg_amd', 'csrc')}",
           "-o", str(exe), os.path.join(ROOT, "tests", "c", "test_contig_decide.cpp")]
    # the sanitizer runtimes are there when a trivial program builds and runs with them; only then is a failure
    # to build the test program the test's own
    probe_c, probe = tmp_path / "probe.cpp", tmp_path / "probe"
    probe_c.write_text("int main() { return 0; }\n")
    flags = ["-fsanitize=address,undefined", "-fno-omit-frame-pointer", "-fno-sanitize-recover=all"]
    pr = subprocess.run([cxx] + flags + ["-o", str(probe), str(probe_c)], stdout=subprocess.PIPE,
                        stderr=subprocess.STDOUT, text=True)
    if pr.returncode != 0 or subprocess.run([str(probe)]).returncode != 0:
        pytest.skip("sanitizer runtime not available: " + pr.stdout[-200:])
    p = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert p.returncode == 0, p.stdout
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:halt_on_error=1")
    r = subprocess.run([str(exe)], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=120, env=env)
    assert r.returncode == 0, r.stdout[-3000:]
    assert "0 failed" in r.stdout
