"""The snapshot's definition and its fixtures (tests/snapshot_ref.py), on the
host: the dictionaries agree with the lattice's analytic arrays, every fixture
meets the condition it exists for (computed from the fixture, not assumed),
and the fixtures tell altered definitions from the true one.  No GPU.

The figures in the comments are what these tests computed when the fixtures
were chosen.  If a seed stops meeting its condition, another seed is chosen:
the condition stays.
"""
import numpy as np
import pytest

import snapshot_ref as R
from parmmg_amd import synth

SCRAMBLED = [n for n in R.FIXTURES if n.startswith(("scr-", "refs-"))]
DROPPED = [n for n in SCRAMBLED if not n.endswith("-d0")]


@pytest.mark.parametrize("kind,n", [(synth.CUBE, 1), (synth.CUBE, 5), (synth.SHELL, 8)])
def test_definition_matches_the_lattice(kind, n):
    bg = synth.lattice(kind, n)
    adja, nonmanifold = R.adjacency(bg.tetv)
    assert not nonmanifold
    np.testing.assert_array_equal(adja, bg.adja)
    triv = R.boundary(bg.tetv, adja)
    np.testing.assert_array_equal(triv, bg.triv)
    np.testing.assert_array_equal(R.tria_adjacency(triv), bg.adjt)
    # a single reference has no interface
    np.testing.assert_array_equal(R.boundary(bg.tetv, adja, np.full(bg.ne, 3, np.int32)), bg.triv)


@pytest.mark.parametrize("name", list(R.FIXTURES))
def test_fixture_is_a_conforming_mesh(name):
    e = R.fixture(name)
    assert e.tetv.dtype == np.int32 and e.tetv.shape == (e.ne, 4)
    assert e.tetv.min() >= 1 and e.tetv.max() <= e.np
    assert (np.diff(np.sort(e.tetv, axis=1), axis=1) > 0).all()  # four distinct ids
    assert not e.nonmanifold
    # the adjacency is an involution and the trias are the faces it leaves open
    k, i = np.nonzero(e.adja)
    back = e.adja[e.adja[k, i] // 4 - 1, e.adja[k, i] % 4]
    np.testing.assert_array_equal(back, 4 * (k + 1) + i)
    if e.tref is None:
        assert e.nt == int((e.adja == 0).sum())
    else:
        assert set(e.tref.tolist()) == {1, 2, 3} and e.nt > int((e.adja == 0).sum())


def test_launch_shape_is_the_source_s():
    """BLOCK, MATCH_VERTS and MATCH_CAP restate constants of pmmg_snapshot.hip"""
    import os
    import re
    src = open(os.path.join(os.path.dirname(R.__file__), "..", "parmmg_amd", "csrc", "pmmg_snapshot.hip")).read()
    assert int(re.search(r"constexpr int kB = (\d+);", src).group(1)) == R.BLOCK
    m = re.search(r"kMatchVerts = (\d+), kMatchCap = (\d+),", src)
    assert (int(m.group(1)), int(m.group(2))) == (R.MATCH_VERTS, R.MATCH_CAP)


def test_lattices_hold_one_position_pair():
    """what the fixtures are for: the generated numbering has the two smallest ids at (0, 1) only"""
    for kind, n in [(synth.CUBE, 5), (synth.SHELL, 8)]:
        assert R.smallest_positions(synth.lattice(kind, n).tetv) == {(0, 1)}


@pytest.mark.parametrize("name", SCRAMBLED)
def test_scrambled_holds_all_twelve_position_pairs(name):
    assert len(R.smallest_positions(R.fixture(name).tetv)) == 12


def test_scrambled_even_permutations_keep_the_orientation():
    bg = synth.lattice(synth.CUBE, 5)
    npv, tetv, xyz, old = R.scrambled_mesh(bg, 4, even=True)
    assert len(R.smallest_positions(tetv)) == 12

    def vol(x, t):
        p = x[t - 1]
        return np.einsum("ij,ij->i", p[:, 1] - p[:, 0], np.cross(p[:, 2] - p[:, 0], p[:, 3] - p[:, 0]))

    np.testing.assert_allclose(vol(xyz, tetv), vol(bg.xyz, bg.tetv)[old], rtol=1e-12)
    assert (vol(xyz, tetv) > 0).all()
    # and the plain one does not
    _, tetv, xyz, _ = R.scrambled_mesh(bg, 4)
    assert (vol(xyz, tetv) < 0).any() and (vol(xyz, tetv) > 0).any()


def test_chunks_on_both_sides_of_the_cap():
    """scr-cube8-d25: chunk max 847, bucket max 66; its chunks are on both
    sides of MATCH_CAP, the dense meshes further above and the sparse below"""
    e = R.fixture("scr-cube8-d25")
    c = R.chunk_sizes(e.np, e.tetv)
    assert c.max() > R.MATCH_CAP and ((c <= R.MATCH_CAP) & (c > 0)).any()
    assert R.bucket_sizes(e.np, e.tetv).max() > 24  # more than any lattice bucket
    assert int(c.sum()) == 4 * e.ne
    for name in SCRAMBLED:
        e = R.fixture(name)
        assert (R.chunk_sizes(e.np, e.tetv) <= R.MATCH_CAP).any(), name
    above = [n for n in SCRAMBLED if R.chunk_sizes(R.fixture(n).np, R.fixture(n).tetv).max() > R.MATCH_CAP]
    assert len(above) >= 5 and len(above) < len(SCRAMBLED), above
    # the lattices stay far below it
    bg = synth.lattice(synth.CUBE, 40)
    assert R.chunk_sizes(bg.np, bg.tetv).max() <= 576 and R.bucket_sizes(bg.np, bg.tetv).max() <= 24


@pytest.mark.parametrize("T,entries", [(255, 765), (256, 768), (257, 771)])
def test_strip_star_chunk_is_exact(T, entries):
    e = R.fixture("star%d" % T)
    assert e.np == T + 26 and e.ne == T
    c = R.chunk_sizes(e.np, e.tetv)
    b = R.bucket_sizes(e.np, e.tetv)
    assert c[0] == entries == 3 * T and b[0] == entries and (b[1:24] == 0).all()
    assert (c[1:] <= 24).all()
    assert (entries > R.MATCH_CAP) == (T == 257)
    # hub = np: an empty bucket for the hub, its faces spread over the strip's
    h = R.fixture("star%d-hub-np" % T)
    bh = R.bucket_sizes(h.np, h.tetv)
    assert h.np == e.np and bh[h.np - 1] == 0 and bh.max() <= 4 and int(bh.sum()) == 4 * T
    assert (h.tetv[:, 0] == h.np).all() and h.nt == e.nt


def test_two_hubs_buckets_and_chunk():
    e = R.fixture("two-hubs-130")
    b = R.bucket_sizes(e.np, e.tetv)
    assert b[0] == b[1] == 390 < R.MATCH_CAP and (b[2:24] == 0).all()
    assert R.chunk_sizes(e.np, e.tetv)[0] == 780 > R.MATCH_CAP
    # the smaller one stays in LDS, with the same {b, c} in the buckets of both hubs
    s = R.fixture("two-hubs-100")
    assert R.chunk_sizes(s.np, s.tetv)[0] == 600 <= R.MATCH_CAP
    for f in (e, s):
        T = f.ne // 2
        np.testing.assert_array_equal(f.tetv[:T, 1:], f.tetv[T:, 1:])
        assert (f.tetv[:T, 0] == 1).all() and (f.tetv[T:, 0] == 2).all()
        assert (f.adja[:, 0] > 0).all()  # every strip triangle is shared by its two tetra


@pytest.mark.parametrize("name", DROPPED)
def test_dropped_tetra_give_edges_of_four_and_six_trias(name):
    """scr-cube6-d30: 1223 edges of two trias, 374 of four, 7 of six"""
    m = R.edge_multiplicities(R.fixture(name).triv)
    assert m.get(2, 0) > 0 and m.get(4, 0) > 0 and m.get(6, 0) > 0, m
    if name.startswith("scr-"):
        assert set(m) <= {2, 4, 6}  # a closed surface: even everywhere


def test_references_give_edges_of_three_and_four_trias_together():
    """refs-cube8-d25: {2: 2592, 3: 213, 4: 645, 5: 42, 6: 45}; the full cube has {2: 792, 3: 48}"""
    m = R.edge_multiplicities(R.fixture("refs-cube8-d25").triv)
    assert m.get(3, 0) > 0 and m.get(4, 0) > 0, m
    m = R.edge_multiplicities(R.fixture("refs-cube6-d0").triv)
    assert m.get(3, 0) > 0, m


@pytest.mark.parametrize("name,ne,inner", [("interior-cube8", 3072, 2352), ("interior-cube10", 6000, 4860)])
def test_interior_first_has_empty_and_full_blocks(name, ne, inner):
    e = R.fixture(name)
    assert e.ne == ne and int((e.adja > 0).all(axis=1).sum()) == inner
    blocks = R.block_candidates(e.adja)
    assert (blocks == 0).sum() == inner // R.BLOCK and (blocks == R.BLOCK).sum() >= 1
    assert blocks[0] == 0 and blocks[inner // R.BLOCK] not in (0, R.BLOCK)  # the block the switch falls in
    # the same tetra in the lattice's own order leave no block empty
    bg = synth.lattice(synth.CUBE, 8)
    assert (R.block_candidates(bg.adja) > 0).all()


def test_prefix_relabels_compactly_and_pads():
    base = R.FIXTURES["scr-cube6-d0"]()
    for ne in (1, 64, 257):
        npv, tetv = R.prefix(base, ne)
        assert tetv.shape == (ne, 4) and set(np.unique(tetv)) == set(range(1, npv + 1))
        np.testing.assert_array_equal(np.argsort(tetv, axis=1), np.argsort(base[1][:ne], axis=1))
        assert R.prefix(base, ne, npv + 3000)[0] == npv + 3000
    assert len(R.smallest_positions(R.prefix(base, 257)[1])) == 12


# ---------------------------------------------------------------- altered definitions
#
# Each of the following is a plausible wrong reading of the conventions.  The
# fixtures named for it must give another result than the true definition:
# a device result that followed the altered rule would not pass.

def test_altered_edge_numbering_differs():
    """edge j taken as (j, j + 1) instead of the edge opposite vertex j"""
    for name in ("one-tetra", "scr-cube6-d0", "star256"):
        e = R.fixture(name)
        alt = R.tria_adjacency(e.triv, edge=lambda tri, j: (tri[j], tri[(j + 1) % 3]))
        assert not np.array_equal(alt, e.adjt), name


@pytest.mark.parametrize("name", DROPPED)
def test_altered_pairing_of_shared_edges_differs(name):
    """pairing whenever at least two trias share the edge"""
    e = R.fixture(name)
    alt = R.tria_adjacency(e.triv, pair=lambda n: n >= 2)
    assert (alt != e.adjt).sum() >= 2 and ((alt != 0) >= (e.adjt != 0)).all()


@pytest.mark.parametrize("name", ["refs-cube6-d0", "refs-cube8-d25"])
def test_altered_interface_rules_differ(name):
    e = R.fixture(name)
    ge = R.boundary(e.tetv, e.adja, e.tref, interface=lambda a, b: a >= b)
    assert ge.shape[0] > e.nt  # every interior face as well
    lt = R.boundary(e.tetv, e.adja, e.tref, interface=lambda a, b: a < b)
    assert lt.shape == e.triv.shape and not np.array_equal(lt, e.triv)  # the same faces from the other side
    assert not np.array_equal(R.boundary(e.tetv, e.adja), e.triv)  # and the references matter at all


@pytest.mark.parametrize("rows", [(0, 1), (1, 2), (2, 3), (0, 3)])
def test_altered_idir_differs(rows):
    """two rows of MMG5_idir exchanged"""
    idir = R.IDIR.copy()
    idir[list(rows)] = idir[list(rows[::-1])]
    for name in ("one-tetra", "scr-cube6-d25", "refs-cube6-d0", "star257", "interior-cube8"):
        e = R.fixture(name)
        assert not np.array_equal(R.boundary(e.tetv, e.adja, e.tref, idir=idir), e.triv), name


@pytest.mark.parametrize("name", ["two-hubs-100", "two-hubs-130"])
def test_altered_face_key_differs(name):
    """a face keyed without its smallest id: {1, b, c} collides with {2, b, c},
    the pair that the bucket term of the LDS hash separates"""
    e = R.fixture(name)
    alt, nonmanifold = R.adjacency(e.tetv, key=lambda f: tuple(sorted(f))[1:])
    assert nonmanifold and not np.array_equal(alt, e.adja)
    # the scrambled meshes hold such pairs within one chunk too
    s = R.fixture("scr-cube8-d50")
    faces = {}
    for t in s.tetv.tolist():
        for i in range(4):
            f = sorted(t[:i] + t[i + 1:])
            faces.setdefault((f[1], f[2], (f[0] - 1) // R.MATCH_VERTS), set()).add(f[0])
    assert sum(len(v) > 1 for v in faces.values()) > 0
