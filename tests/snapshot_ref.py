"""The background snapshot by its definition, and the meshes it is tested on.

The three operations of include/parmmg_hip.h ("Background snapshot on the
device") stated with dictionaries, from the conventions alone (Mmg's
MMG3D_hashTetra / MMG5_chkBdryTria / MMG3D_hashTria, restated):

  adjacency(tetv)              face i of a tetra is the face opposite vertex
                               i; two tetra share a face when its sorted ids
                               agree; adja = 4 k' + i', 0 on the boundary
  boundary(tetv, adja, tref)   the faces with adja == 0, or towards a
                               neighbour of smaller reference, in (tetra,
                               face) order, vertices v[MMG5_idir[i]]
  tria_adjacency(triv)         edge j is the edge opposite local vertex j;
                               adjt = 3 t' + j' when exactly two trias share
                               the edge, else 0

Nothing here knows of buckets, waves or chunks, and nothing reads the
lattice's analytic arrays.  The keyword arguments of the three functions
exist for tests/test_snapshot_ref_host.py only: it passes altered rules and
shows that the fixtures below tell them from the true ones.

The fixtures are meshes whose numbering and sizes reach the parts of
pmmg_snapshot.hip a lattice in its generated numbering never does; the
measures at the end (bucket and chunk sizes, positions of the smallest ids,
edge multiplicities, candidates per block) are what the host tests compute to
show that each fixture does.  Host only: numpy and the lattice generator.
"""
from __future__ import annotations

import functools
from collections import Counter

import numpy as np

from parmmg_amd import synth
from parmmg_amd.transfer import pack_tet8  # noqa: F401  (tet8 = pack_tet8(tetv, adja))

IDIR = np.array([[1, 2, 3], [0, 3, 2], [0, 1, 3], [0, 2, 1]])  # MMG5_idir

# pmmg_snapshot.hip's launch shape, restated for the measures below
BLOCK = 256        # kB: tetra per block of the boundary compaction
MATCH_VERTS = 24   # kMatchVerts: vertices (buckets) per block of k_face_match
MATCH_CAP = 768    # kMatchCap: entries a chunk stages in LDS; above, matched in place


def _sorted_face(ids):
    return tuple(sorted(ids))


def adjacency(tetv, key=_sorted_face):
    """(adja, nonmanifold): MMG3D_hashTetra's result by a dictionary of faces
    keyed by their sorted ids (face i opposite vertex i); nonmanifold when a
    face belongs to more than two tetra (its entries then stay 0)."""
    faces = {}
    for k, t in enumerate(np.asarray(tetv).tolist()):
        for i in range(4):
            faces.setdefault(key(t[:i] + t[i + 1:]), []).append(4 * (k + 1) + i)
    adja = np.zeros(np.asarray(tetv).shape, np.int32)
    nonmanifold = False
    for codes in faces.values():
        if len(codes) == 2:
            a, b = codes
            adja[a // 4 - 1, a % 4], adja[b // 4 - 1, b % 4] = b, a
        nonmanifold |= len(codes) > 2
    return adja, nonmanifold


def _larger(ref, ref_neighbour):
    return ref > ref_neighbour


def boundary(tetv, adja, tref=None, idir=IDIR, interface=_larger):
    """triv: the faces without a neighbour and, with references, the
    interface faces seen from the larger reference (MMG5_chkBdryTria's rule
    for an old mesh without input trias), in (tetra, face) order, oriented by
    MMG5_idir."""
    tetv, adja = np.asarray(tetv), np.asarray(adja)
    rows = []
    for k in range(tetv.shape[0]):
        for i in range(4):
            c = int(adja[k, i])
            if c == 0 or (tref is not None and interface(int(tref[k]), int(tref[c // 4 - 1]))):
                rows.append(tetv[k, idir[i]])
    return np.array(rows, np.int32).reshape(-1, 3)


def _opposite_edge(tri, j):
    return tri[(j + 1) % 3], tri[(j + 2) % 3]


def _exactly_two(n):
    return n == 2


def tria_adjacency(triv, edge=_opposite_edge, pair=_exactly_two):
    """MMG3D_hashTria's adjt: edge j (opposite local vertex j) paired only
    when exactly two trias share it"""
    edges = {}
    for t, tri in enumerate(np.asarray(triv).tolist()):
        for j in range(3):
            edges.setdefault(tuple(sorted(edge(tri, j))), []).append(3 * (t + 1) + j)
    adjt = np.zeros(np.asarray(triv).shape, np.int32)
    for codes in edges.values():
        if pair(len(codes)):
            a, b = codes[:2]
            adjt[a // 3 - 1, a % 3], adjt[b // 3 - 1, b % 3] = b, a
    return adjt


# ---------------------------------------------------------------- fixtures
#
# Every generator is seeded and returns (np, tetv[, tref]) with 1-based int32
# ids.  Connectivity is all the snapshot reads, and any subset of a conforming
# mesh is conforming, so tetra may be dropped and ids renamed freely.

_EVEN = np.array([p for p in np.ndindex(4, 4, 4, 4) if len(set(p)) == 4 and
                  sum(p[a] > p[b] for a in range(4) for b in range(a + 1, 4)) % 2 == 0])  # the 12 even permutations


def scrambled_mesh(bg, seed, drop=0.0, even=False):
    """(np, tetv, xyz, old): a lattice with a random share `drop` of its tetra
    removed, vertex ids permuted, tetra order permuted, and the four vertices
    of every tetra permuted independently (even: by even permutations only,
    which keeps every tetra's orientation; they still reach all 12 positions of
    the two smallest ids).  xyz are the coordinates under the new ids and
    old[j] the lattice row of new tetra j."""
    rng = np.random.default_rng(seed)
    old = np.nonzero(rng.random(bg.ne) >= drop)[0]
    pv = rng.permutation(bg.np) + 1  # lattice vertex v -> id pv[v - 1]
    old = old[rng.permutation(old.size)]
    tetv = pv[bg.tetv[old] - 1]
    if even:
        order = _EVEN[rng.integers(0, 12, old.size)]
    else:
        order = np.argsort(rng.random((old.size, 4)), axis=1)
    tetv = np.take_along_axis(tetv, order, axis=1)
    xyz = np.empty_like(bg.xyz)
    xyz[pv - 1] = bg.xyz
    return bg.np, np.ascontiguousarray(tetv, np.int32), xyz, old


def scrambled(bg, seed, drop=0.0, refs=0):
    """(np, tetv), or with refs (np, tetv, tref): tref numbers `refs` slabs of
    equal thickness along x, by the tetra's centroid."""
    npv, tetv, xyz, _ = scrambled_mesh(bg, seed, drop)
    if not refs:
        return npv, tetv
    cx = xyz[tetv - 1, 0].mean(axis=1)
    tref = (np.floor(refs * (cx - cx.min()) / np.ptp(cx) * 0.999) + 1).astype(np.int32)
    return npv, tetv, tref


def interior_first(bg):
    """The lattice with every tetra that has no boundary face placed first:
    whole 256-blocks without a candidate of the boundary compaction, followed
    by blocks full of them."""
    inner = (bg.adja > 0).all(axis=1)
    order = np.concatenate([np.nonzero(inner)[0], np.nonzero(~inner)[0]])
    return bg.np, np.ascontiguousarray(bg.tetv[order], np.int32)


def _strip(T, hub):
    """the T triangles (v_i, v_i+1, v_i+2) of a strip over T + 2 consecutive ids, np = T + 26"""
    first = 24 if hub == T + 26 else 25  # (the hub np takes the strip's last id)
    v = np.arange(first, first + T + 2, dtype=np.int32)
    return np.stack([v[:-2], v[1:-1], v[2:]], axis=1)


def strip_star(T, hub=1):
    """T tetra (hub, a, b, c) over a triangle strip on the ids 25 ... T + 26,
    np = T + 26.  With hub 1 the first chunk of 24 vertices holds the hub's
    bucket alone, of exactly 3 T entries, and every other chunk at most 24.
    hub = np: the hub is the largest id, its bucket is empty and its faces are
    spread over the strip's buckets."""
    npv = T + 26
    assert hub in (1, npv)
    tri = _strip(T, hub)
    return npv, np.ascontiguousarray(np.hstack([np.full((T, 1), hub, np.int32), tri]))


def two_hubs(T):
    """Two stars over one strip, on hubs 1 and 2 (a double cone: each strip
    triangle is shared by its two tetra).  The buckets of both hubs are in the
    first chunk, with the same {b, c} in both."""
    tri = _strip(T, 1)
    one, two = np.full((T, 1), 1, np.int32), np.full((T, 1), 2, np.int32)
    return T + 26, np.ascontiguousarray(np.vstack([np.hstack([one, tri]), np.hstack([two, tri])]))


def prefix(mesh, ne, np_pad=None):
    """The first ne tetra of a mesh, ids relabelled compactly (in their
    order), with np = np_pad (None: the largest id).  Vertices past the
    largest id are unused and their buckets empty."""
    ids, inv = np.unique(mesh[1][:ne], return_inverse=True)
    tetv = np.ascontiguousarray(inv.reshape(-1, 4) + 1, np.int32)
    npv = ids.size if np_pad is None else int(np_pad)
    assert npv >= ids.size
    return npv, tetv


ONE_TETRA = (4, np.array([[3, 1, 4, 2]], np.int32))


# name -> generator of (np, tetv[, tref]); the seeds are fixed here, and the
# conditions each fixture exists for are computed in tests/test_snapshot_ref_host.py
FIXTURES = {
    "one-tetra": lambda: ONE_TETRA,
    "scr-cube6-d0": lambda: scrambled(synth.lattice(synth.CUBE, 6), 5),
    "scr-cube6-d25": lambda: scrambled(synth.lattice(synth.CUBE, 6), 6, 0.25),
    "scr-cube6-d30": lambda: scrambled(synth.lattice(synth.CUBE, 6), 3, 0.3),
    "scr-cube6-d50": lambda: scrambled(synth.lattice(synth.CUBE, 6), 7, 0.5),
    "scr-cube8-d0": lambda: scrambled(synth.lattice(synth.CUBE, 8), 10),
    "scr-cube8-d25": lambda: scrambled(synth.lattice(synth.CUBE, 8), 11, 0.25),
    "scr-cube8-d50": lambda: scrambled(synth.lattice(synth.CUBE, 8), 12, 0.5),
    "scr-shell8-d0": lambda: scrambled(synth.lattice(synth.SHELL, 8), 20),
    "scr-shell8-d25": lambda: scrambled(synth.lattice(synth.SHELL, 8), 21, 0.25),
    "scr-shell8-d50": lambda: scrambled(synth.lattice(synth.SHELL, 8), 22, 0.5),
    "scr-cube10-d0": lambda: scrambled(synth.lattice(synth.CUBE, 10), 30),
    "refs-cube6-d0": lambda: scrambled(synth.lattice(synth.CUBE, 6), 40, 0.0, refs=3),
    "refs-cube8-d25": lambda: scrambled(synth.lattice(synth.CUBE, 8), 41, 0.25, refs=3),
    "interior-cube8": lambda: interior_first(synth.lattice(synth.CUBE, 8)),
    "interior-cube10": lambda: interior_first(synth.lattice(synth.CUBE, 10)),
    "star255": lambda: strip_star(255),
    "star256": lambda: strip_star(256),
    "star257": lambda: strip_star(257),
    "star255-hub-np": lambda: strip_star(255, 255 + 26),
    "star256-hub-np": lambda: strip_star(256, 256 + 26),
    "star257-hub-np": lambda: strip_star(257, 257 + 26),
    "two-hubs-130": lambda: two_hubs(130),  # 390 + 390 entries: matched in place
    "two-hubs-100": lambda: two_hubs(100),  # 300 + 300: staged in LDS, the same {b, c} in two buckets
}


class Expected:
    """A fixture with its arrays by the definition (read-only: shared among tests)"""

    def __init__(self, name, npv, tetv, tref=None):
        self.name, self.np, self.tetv, self.tref = name, int(npv), tetv, tref
        self.adja, self.nonmanifold = adjacency(tetv)
        self.tet8 = pack_tet8(tetv, self.adja)
        self.triv = boundary(tetv, self.adja, tref)
        self.adjt = tria_adjacency(self.triv)
        for a in (self.tetv, self.tref, self.adja, self.tet8, self.triv, self.adjt):
            if a is not None:
                a.setflags(write=False)

    ne = property(lambda self: self.tetv.shape[0])
    nt = property(lambda self: self.triv.shape[0])


@functools.lru_cache(maxsize=None)
def fixture(name):
    return Expected(name, *FIXTURES[name]())


def expected(npv, tetv, tref=None, name=""):
    """the arrays of a mesh that is not in FIXTURES (a prefix, a permuted copy)"""
    return Expected(name, npv, np.ascontiguousarray(tetv, np.int32), tref)


# ---------------------------------------------------------------- measures

def smallest_positions(tetv):
    """the set of (position of the smallest id, position of the second smallest) over the tetra"""
    order = np.argsort(tetv, axis=1)
    return set(zip(order[:, 0].tolist(), order[:, 1].tolist()))


def bucket_sizes(npv, tetv):
    """faces per vertex bucket: a tetra puts the three faces holding its
    smallest id there, and the fourth under its second smallest"""
    s = np.sort(tetv, axis=1)
    return np.bincount(s[:, 0] - 1, minlength=npv) * 3 + np.bincount(s[:, 1] - 1, minlength=npv)


def chunk_sizes(npv, tetv):
    """entries per block of k_face_match: MATCH_VERTS consecutive buckets"""
    b = bucket_sizes(npv, tetv)
    pad = (-b.size) % MATCH_VERTS
    return np.concatenate([b, np.zeros(pad, b.dtype)]).reshape(-1, MATCH_VERTS).sum(axis=1)


def edge_multiplicities(triv):
    """{number of trias on an edge: number of such edges}"""
    edges = Counter()
    for tri in np.asarray(triv).tolist():
        for j in range(3):
            edges[tuple(sorted(_opposite_edge(tri, j)))] += 1
    return dict(sorted(Counter(edges.values()).items()))


def block_candidates(adja, tref=None):
    """tetra with a boundary face per 256-block of the boundary compaction"""
    adja = np.asarray(adja)
    cand = adja == 0
    if tref is not None:
        cand |= tref[:, None] > tref[np.maximum(adja // 4 - 1, 0)]
    cand = cand.any(axis=1)
    pad = (-cand.size) % BLOCK
    return np.concatenate([cand, np.zeros(pad, bool)]).reshape(-1, BLOCK).sum(axis=1)


def measures(e):
    """what the pull request's summary lists per fixture"""
    blocks = block_candidates(e.adja, e.tref)
    full = np.minimum(BLOCK, e.ne - BLOCK * np.arange(blocks.size))
    return dict(ne=e.ne, np=e.np, nt=e.nt, chunk_max=int(chunk_sizes(e.np, e.tetv).max()),
                bucket_max=int(bucket_sizes(e.np, e.tetv).max()), edges=edge_multiplicities(e.triv),
                blocks=int(blocks.size), blocks_empty=int((blocks == 0).sum()), blocks_full=int((blocks == full).sum()))


if __name__ == "__main__":
    for fx in FIXTURES:
        print(fx, measures(fixture(fx)))
