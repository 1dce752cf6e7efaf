"""The interpolation of the transfer step in 50-digit arithmetic, with forward
error bounds for its binary64 evaluation, and the seeded inputs the CPU and
GPU tests share (tests/test_highprec_interp_host.py,
tests/test_gpu_interp_highprec.py).  The companion of tests/highprec.py, in
its style.

Every function is written from the mathematical definition (a ratio of
determinants, an orthogonal projection, sum_i phi_i f_i, (sum_i phi_i M_i^-1)^-1
with the inverse as adjugate over determinant of the full 3 x 3 matrix), not in
the operation order of oracle/pmmg_oracle.c or of the kernels, and takes its
inputs as the exact binary64 values.  It returns (value, bound): bound is what a
binary64 evaluation of the operation may be off by, to first order, with u =
2^-53: every product and sum evaluated with absolute values, the coordinates'
and the first inversions' errors propagated through what follows.  No constant
is fitted to an output: each docstring gives the operation counts.

Two parts of the definition are not mathematics but MMG5_invmat's text, and
are restated as such: the diagonal shortcut (off-diagonals all below MMG5_EPS:
the inverse is 1 / diagonal, the off-diagonals are dropped) and its failures
(|det| < MMG5_EPSD2; the zero matrix, which the shortcut in front of that test
catches first, so that 1 / 0 is what it gives).  Which vertices a hit kind
interpolates over is src/interpmesh_pmmg.c:563-636, restated in rule_rows()."""
from __future__ import annotations

import functools

import numpy as np

import highprec as H
from highprec import U, mp

MMG_EPS = H.MMG_EPS
EPSD2 = H.EPSD2
ZERO = mp.mpf(0)

# MMG5_idir: the vertices of face f (the face opposite vertex f); the first is the
# one PMMG_barycoord3d_compute measures the point from
IDIR = ((1, 2, 3), (0, 3, 2), (0, 1, 3), (0, 2, 1))
for _f in range(4):
    assert sorted(IDIR[_f]) == [i for i in range(4) if i != _f]

VOL_WALK, VOL_EXHAUST, VOL_CLOSEST = 1, 2, 3
BDY_FACE, BDY_EDGE, BDY_VERTEX, BDY_EXHAUST = 4, 5, 6, 9


def _v(x):
    return [mp.mpf(float(t)) for t in x]


def _sub(a, b):
    """b - a"""
    return [y - x for x, y in zip(a, b)]


def _cross(a, b):
    return [a[1] * b[2] - a[2] * b[1], a[2] * b[0] - a[0] * b[2], a[0] * b[1] - a[1] * b[0]]


def _dot(a, b):
    return a[0] * b[0] + a[1] * b[1] + a[2] * b[2]


def _abs(a):
    return [abs(t) for t in a]


def _det3(a, b, c):
    return _dot(a, _cross(b, c))


def _cross_abs(a, b):
    """the cross product's components with both products made absolute"""
    a, b = _abs(a), _abs(b)
    return [a[1] * b[2] + a[2] * b[1], a[2] * b[0] + a[0] * b[2], a[0] * b[1] + a[1] * b[0]]


# ---------------------------------------------------------------- coordinates

def tet_coords(p, x, exchange=None):
    """Barycentric coordinates of x in the tetra p[4]: phi_i = det(p with p_i
    replaced by x) / det(p), each a 3 x 3 determinant of differences.
    Returns ([4] phi, [4] bounds).

    Bound u (8 A_f / |D| + |phi_f| (8 P / |D| + 1)).  The binary64 operation forms
    -(x - c) . n_f / D, c the first vertex of face f in MMG5_idir, n_f the face's
    cross product, D the triple product.  Each of the six products of either
    determinant carries 3 rounded differences, 2 multiplications and at most 3
    additions: 8 u A_f on the numerator (A_f: the six products' moduli, from c)
    and 8 u P on D; the quotient rounds once, the sign is exact.

    exchange: (i, j), the altered variant of the harness' self-check."""
    p = [_v(r) for r in p]
    x = _v(x)
    D = _det3(_sub(p[0], p[1]), _sub(p[0], p[2]), _sub(p[0], p[3]))
    P = H._perm(_sub(p[0], p[1]), _sub(p[0], p[2]), _sub(p[0], p[3]))
    phi, bnd = [], []
    for f in range(4):
        q = list(p)
        q[f] = x
        v = _det3(_sub(q[0], q[1]), _sub(q[0], q[2]), _sub(q[0], q[3])) / D
        a, b, c = (p[i] for i in IDIR[f])
        A = H._perm(_sub(a, x), _sub(a, b), _sub(a, c))
        phi.append(v)
        bnd.append(U * (8 * A / abs(D) + abs(v) * (8 * P / abs(D) + 1)))
    if exchange:
        i, j = exchange
        phi[i], phi[j] = phi[j], phi[i]
    return phi, bnd


def tria_coords(p, x, project=True):
    """x against the tria p[3]: with N = (p1 - p0) x (p2 - p0) and n = N / |N|,
    the signed normal distance dist = (x - p0) . n and the barycentric coordinates
    of the projection x - dist n, written without it: phi_i = ((a - x) x (c - x)) . N
    / |N|^2, a and c the vertices (i + 1) % 3 and (i + 2) % 3 (the normal part of a
    - x and c - x drops out of a triple product with N).
    Returns ([3] phi, [3] bounds, dist, dist's bound).

    The binary64 operation (PMMG_barycoord2d_compute) goes through the unit
    normal, the distance and the projected point, and the bound follows it:
      N_k: 2 differences, 1 product, 1 subtraction: 4 u Nabs_k;
      q = |N|: |dN| and 3 u q (squares, two additions, the root);
      n_k = N_k (1 / q): dN_k / q + |n_k| (dq / q + 2 u);
      dist: sum |x - p0| dn and 4 u sum |x - p0| |n| (difference, product, 2 additions);
      proj_k = x_k - dist n_k: |n_k| ddist + |dist| dn_k + u |dist n_k| + u |proj_k|
        (the last is the coordinates' spacing: it dominates far from the origin);
      a - proj, c - proj: dproj + u |.|;
      the area (a - proj) x (c - proj) . n: the differences' and n's errors through
        every product, and 5 u of the products' moduli (2 products, the
        subtraction, 2 additions);
      phi = area / q: darea / q + |phi| (dq / q + u).

    project=False is the altered variant of the harness' self-check: the
    sub-triangles' areas taken in space at x itself, |(a - x) x (c - x)| / |N|.
    (Leaving out the projected point alone changes nothing: see above.)"""
    p = [_v(r) for r in p]
    x = _v(x)
    e1, e2 = _sub(p[0], p[1]), _sub(p[0], p[2])
    N = _cross(e1, e2)
    q2 = _dot(N, N)
    q = mp.sqrt(q2)
    n = [t / q for t in N]
    d0 = _sub(p[0], x)
    dist = _dot(d0, n)
    dN = [4 * U * t for t in _cross_abs(e1, e2)]
    dq = mp.sqrt(_dot(dN, dN)) + 3 * U * q
    dn = [dN[k] / q + abs(n[k]) * (dq / q + 2 * U) for k in range(3)]
    ddist = _dot(_abs(d0), dn) + 4 * U * _dot(_abs(d0), _abs(n))
    proj = [x[k] - dist * n[k] for k in range(3)]
    dproj = [abs(n[k]) * ddist + abs(dist) * dn[k] + U * abs(dist * n[k]) + U * abs(proj[k]) for k in range(3)]
    phi, bnd = [], []
    for i in range(3):
        a, c = p[(i + 1) % 3], p[(i + 2) % 3]
        if project:
            v = _dot(_cross(_sub(x, a), _sub(x, c)), N) / q2
        else:
            w = _cross(_sub(x, a), _sub(x, c))
            v = mp.sqrt(_dot(w, w)) / q
        ab, ac = _abs(_sub(proj, a)), _abs(_sub(proj, c))
        dab = [dproj[k] + U * ab[k] for k in range(3)]
        dac = [dproj[k] + U * ac[k] for k in range(3)]
        cab = _cross_abs(ab, ac)
        darea = _dot(_cross_abs(dab, ac), _abs(n)) + _dot(_cross_abs(ab, dac), _abs(n)) + _dot(cab, dn) \
            + 5 * U * _dot(cab, _abs(n))
        phi.append(v)
        bnd.append(darea / q + abs(v) * (dq / q + U))
    return phi, bnd, dist, ddist


def border(phi):
    """PMMG_barycoord_isBorder on a tria's coordinates: (kind, loc).  With the
    coordinates sorted ascending (ties in index order): smallest < MMG5_EPS and
    second < MMG5_EPS: a vertex hit on the largest's vertex; smallest alone: an
    edge hit on the smallest's edge (the edge opposite that vertex); else a face
    hit."""
    order = sorted(range(3), key=lambda i: (phi[i], i))
    if phi[order[0]] < MMG_EPS:
        if phi[order[1]] < MMG_EPS:
            return BDY_VERTEX, order[2]
        return BDY_EDGE, order[0]
    return BDY_FACE, 0


def nearest_vertex(p, x):
    """PMMG_barycoord*_getClosest: the unit coordinate on the nearest vertex"""
    p = [_v(r) for r in p]
    x = _v(x)
    d = [mp.sqrt(sum(t * t for t in _sub(r, x))) for r in p]
    it = min(range(len(p)), key=lambda i: (d[i], i))
    return [mp.mpf(1) if i == it else ZERO for i in range(len(p))]


# ---------------------------------------------------------------- interpolators

def interp_p1(phi, dphi, rows):
    """sum_i phi_i f_i over the vertices' rows (1 or 3 doubles each).
    Bound sum dphi_i |f_i| + n u sum |phi_i f_i| per component: the coordinates'
    bounds, then one product and at most n - 1 rounded additions per term (the
    sum starts from an exact 0)."""
    rows = [_v(r) for r in rows]
    n = len(rows)
    val, bnd = [], []
    for j in range(len(rows[0])):
        val.append(sum(phi[i] * rows[i][j] for i in range(n)))
        bnd.append(sum(dphi[i] * abs(rows[i][j]) for i in range(n)) +
                   n * U * sum(abs(phi[i] * rows[i][j]) for i in range(n)))
    return val, bnd


SYM = ((0, 1, 2), (1, 3, 4), (2, 4, 5))  # where M[i][j] sits in (m11 m12 m13 m22 m23 m33)
PAIR = ((0, 0), (0, 1), (0, 2), (1, 1), (1, 2), (2, 2))


def invmat(m, dm=None, shortcut=True):
    """MMG5_invmat of (m11 m12 m13 m22 m23 m33) given as mpf, each known to
    within dm.  Returns ([6] inverse, [6] bounds, max |off-diagonal|), or None
    where MMG5_invmat returns 0.

    The definition: below MMG5_EPS on every off-diagonal the inverse of the
    diagonal alone, the off-diagonals exactly 0 (shortcut=False, the self-check's
    altered variant, ignores this); else adj(M) / det(M), failing on the zero matrix
    and on |det| < MMG5_EPSD2.

    Bounds.  Shortcut: dm_k / m_k^2 + u / |m_k|; 0 on the off-diagonals.  Else,
    with C_k = m_a m_b - m_c m_d the cofactor of entry k: dC_k = 2 u (|m_a m_b| +
    |m_c m_d|) (product, subtraction) plus the inputs' dm through the four
    factors; det = m_0 C_0 + m_1 C_1 + m_2 C_2: sum (|m_i| dC_i + dm_i |C_i|) + 3 u
    sum |m_i C_i| (product, two additions); inverse_k = C_k (1 / det): dC_k / |det|
    + |inverse_k| (ddet / |det| + 2 u)."""
    dm = dm or [ZERO] * 6
    off = max(abs(m[1]), abs(m[2]), abs(m[4]))
    if shortcut and off < MMG_EPS:
        val = [1 / m[0] if m[0] != 0 else mp.inf, ZERO, ZERO, 1 / m[3] if m[3] != 0 else mp.inf, ZERO,
               1 / m[5] if m[5] != 0 else mp.inf]
        bnd = [ZERO] * 6
        for k in (0, 3, 5):
            bnd[k] = dm[k] / (m[k] * m[k]) + U / abs(m[k]) if m[k] != 0 else ZERO
        return val, bnd, off
    if max(abs(t) for t in m) == 0:
        return None
    M = [[m[SYM[i][j]] for j in range(3)] for i in range(3)]
    dM = [[dm[SYM[i][j]] for j in range(3)] for i in range(3)]
    C, dC = [[None] * 3 for _ in range(3)], [[None] * 3 for _ in range(3)]
    for i in range(3):
        for j in range(3):
            r0, r1 = [r for r in range(3) if r != i]
            c0, c1 = [c for c in range(3) if c != j]
            sgn = -1 if (i + j) % 2 else 1
            C[i][j] = sgn * (M[r0][c0] * M[r1][c1] - M[r0][c1] * M[r1][c0])
            dC[i][j] = 2 * U * (abs(M[r0][c0] * M[r1][c1]) + abs(M[r0][c1] * M[r1][c0])) + \
                dM[r0][c0] * abs(M[r1][c1]) + abs(M[r0][c0]) * dM[r1][c1] + \
                dM[r0][c1] * abs(M[r1][c0]) + abs(M[r0][c1]) * dM[r1][c0]
    det = sum(M[0][j] * C[0][j] for j in range(3))
    if abs(det) < EPSD2:
        return None
    ddet = sum(abs(M[0][j]) * dC[0][j] + dM[0][j] * abs(C[0][j]) for j in range(3)) + \
        3 * U * sum(abs(M[0][j] * C[0][j]) for j in range(3))
    val = [C[j][i] / det for i, j in PAIR]
    bnd = [dC[j][i] / abs(det) + abs(v) * (ddet / abs(det) + 2 * U) for (i, j), v in zip(PAIR, val)]
    return val, bnd, off


def interp_tensor(phi, dphi, inverses, linear_rows=None, shortcut=True):
    """(sum_i phi_i M_i^-1)^-1 over 4, 3 or 2 vertices: inverses[i] = invmat(M_i)
    (None: that inversion failed).  Returns ([6] value, [6] bounds, max
    |off-diagonal| of the sum), or (None, None, off) where the reference leaves the
    row untouched (an inversion failed).

    The sum: dphi_i |M_i^-1| + |phi_i| d(M_i^-1) + n u sum |phi_i M_i^-1| per
    component (one product and at most n - 1 additions per term); then invmat's
    bound with that as its input's error.

    linear_rows: the self-check's altered variant sum_i phi_i M_i."""
    n = len(phi)
    if linear_rows is not None:
        rows = [_v(r) for r in linear_rows]
        return [sum(phi[i] * rows[i][s] for i in range(n)) for s in range(6)], [ZERO] * 6, ZERO
    if any(v is None for v in inverses):
        return None, None, ZERO
    mint = [sum(phi[i] * inverses[i][0][s] for i in range(n)) for s in range(6)]
    dmint = [sum(dphi[i] * abs(inverses[i][0][s]) + abs(phi[i]) * inverses[i][1][s] for i in range(n)) +
             n * U * sum(abs(phi[i] * inverses[i][0][s]) for i in range(n)) for s in range(6)]
    out = invmat(mint, dmint, shortcut)
    off = max(abs(mint[1]), abs(mint[2]), abs(mint[4]))
    if out is None:
        return None, None, off
    return out[0], out[1], off


def edge_ends(l, altered=False):
    """PMMG_interp2bar on edge l of a tria: the vertices MMG5_inxt2[l] and
    MMG5_iprv2[l], with their own (unnormalised) coordinates.  altered: (l, l + 1),
    the self-check's variant."""
    return (l, (l + 1) % 3) if altered else ((l + 1) % 3, (l + 2) % 3)


# ---------------------------------------------------------------- shared inputs
#
# A soup of disjoint elements: every tetra and every tria has vertices of its
# own, no neighbour (adja = adjt = 0) and a cell of a 2.0-spaced lattice to
# itself, so a query placed in an element can only be found in that one: with a
# point map naming one of its vertices the walk starts and ends there, without
# one the exhaustive search finds it.  The background and the queries are
# built in the unit frame and moved to the three frames as x -> s x + t.

FRAMES = ((1.0, 0.0), (1e-4, 1e3), (1e3, 0.0))
assert all(f in H.FRAMES for f in FRAMES)
HAUSD = 0.01
SPACING = 2.0
ISO = ("met1", "s0", "s1", "s2", "s3", "s4", "vec")
TENSOR = ("met6", "ten6")
SIZE = dict(met1=1, met6=6, ten6=6, s0=1, s1=1, s2=1, s3=1, s4=1, vec=3)
AFFINE = (1.5, 2.0, -0.75, 0.5)  # s0 = a0 + a . x at the unit frame's vertices
TENSOR_CLASSES = ("same-rotation", "rotation-per-vertex", "stretch-1e2", "stretch-1e4", "shortcut-input",
                  "shortcut-mint")
N_TET, N_TRI = 156, 96
TET_QUERY = ("interior", "interior", "c-5e-7", "c0", "c+5e-7", "c1e-3", "edge", "vertex")
TRI_QUERY = ("face", "face", "face", "edge", "edge", "vertex")
N_OUTSIDE = 12


def _in_gap(t):
    off = np.max(np.abs(np.asarray(t)[..., [1, 2, 4]]), axis=-1)
    return bool(np.any((off > 0.9e-6) & (off < 1.1e-6)))


def _tensor_rows(rng, cls, nv):
    """nv vertex tensors of one element of class cls (drawn again while one has
    its largest off-diagonal between 0.9e-6 and 1.1e-6)"""
    while True:
        if cls == "same-rotation":
            Q, lam = H.tensor(rng, 0.5, 4.0)
            rows = [H.sym6((Q * (lam * (1.0 + rng.uniform(-0.3, 0.3, 3)))) @ Q.T) for _ in range(nv)]
        elif cls in ("rotation-per-vertex", "stretch-1e2", "stretch-1e4"):
            hi = dict([("rotation-per-vertex", 9.0), ("stretch-1e2", 1e2), ("stretch-1e4", 1e4)])[cls]
            rows = []
            for _ in range(nv):
                Q, lam = H.tensor(rng, 1.0, hi)  # eigenvalues log-uniform over the stretch
                rows.append(H.sym6((Q * lam) @ Q.T))
        elif cls == "shortcut-input":
            # diagonals of 3e-6 to 1e-5 beside off-diagonals of 0.5e-6 (dropped) or 2e-6 (kept), per vertex
            rows = []
            for _ in range(nv):
                d = rng.uniform(3e-6, 1e-5, 3)
                o = rng.choice([0.5e-6, 2e-6]) * rng.choice([-1.0, 1.0], 3) * rng.uniform(0.8, 1.0, 3)
                rows.append(np.array([d[0], o[0], o[1], d[1], o[2], d[2]]))
        else:
            # M_i = W_i^-1 with W_i's off-diagonals all at one of 0.5e-6 / 2e-6 over the element: the
            # interpolated inverse sum phi_i W_i has them there too, on one side of the switch; the diagonals
            # of W_i are small enough that M_i's own off-diagonals stay above it
            o = rng.choice([0.5e-6, 2e-6]) * rng.choice([-1.0, 1.0], 3)
            rows = []
            for _ in range(nv):
                d = rng.uniform(0.2, 0.5, 3)
                W = np.array([[d[0], o[0], o[1]], [o[0], d[1], o[2]], [o[1], o[2], d[2]]])
                rows.append(H.sym6(np.linalg.inv(W)))
        rows = np.array(rows)
        if not _in_gap(rows):
            return rows


def _tet_shape(rng, k):
    kind = ("regular", "normal", "normal", "sliver1e-03", "normal", "sliver1e-05")[k % 6]
    if kind == "regular":
        p = (H.REG * 0.1) @ H._rotation(rng).T
    elif kind == "normal":
        p = rng.normal(size=(4, 3)) * 0.1
    else:
        p = H._sliver(rng, float(kind[6:])) * 0.1
    return H._orient(p), kind


def _phimin_frames(p, x):
    """the smallest barycentric coordinate of x in the tetra p, in binary64, as each of FRAMES holds them"""
    out = []
    for s, t in FRAMES:
        pp, xx = p * s + t, x * s + t
        b = np.linalg.solve((pp[1:] - pp[0]).T, xx - pp[0])
        out.append(min(1.0 - b.sum(), b.min()))
    return out


def _inv6(m):
    """MMG5_invmat in numpy (for drawing the inputs only)"""
    if np.abs(m[[1, 2, 4]]).max() < 1e-6:
        return np.array([1.0 / m[0], 0.0, 0.0, 1.0 / m[3], 0.0, 1.0 / m[5]])
    M = np.array([[m[0], m[1], m[2]], [m[1], m[3], m[4]], [m[2], m[4], m[5]]])
    with np.errstate(all="ignore"):
        return H.sym6(np.linalg.inv(M)) if abs(np.linalg.det(M)) > 0 else np.full(6, np.nan)


def _near_switch(sol, ids, ph, check):
    """whether sum_i ph_i M_i^-1 of met6 / ten6 (check: which of them) over the vertices ids, or over an
    edge's two, has its largest off-diagonal between 0.2e-6 and 5e-6: a tiny coordinate times a large inverse
    can land there, and the frames move tiny coordinates by a few 1e-9, hence the wide berth.  (The class
    built to sit at 0.5e-6 and 2e-6 is not checked: its sums are there by construction.)"""
    for name, on in zip(TENSOR, check):
        if not on:
            continue
        inv = np.array([_inv6(np.asarray(sol[name][i - 1])) for i in ids])
        subsets = [list(range(len(ids)))]
        if len(ids) == 3 and (np.abs(ph) < 1e-6).sum() == 1:  # an edge hit: the metric over the edge's two ends
            subsets.append([i for i in range(3) if abs(ph[i]) >= 1e-6])
        for sub in subsets:
            sub = np.array(sub)
            sure = sub[np.abs(ph[sub]) >= 1e-6]
            off = np.abs((ph[sure, None] * inv[sure]).sum(0)[[1, 2, 4]]).max()
            # a coordinate of 0 is 1e-11 or more once a frame has rounded the point: beside an inverse of 1e5 that
            # decides the switch, unless the rest of the sum is clear of it or that vertex adds no off-diagonal
            loose = np.abs(inv[np.setdiff1d(sub, sure)][:, [1, 2, 4]]).max() > 0 if sure.size < sub.size else False
            if 0.2e-6 < off < 5e-6 or (loose and off < 5e-6):
                return True
    return False


def _closest_values(xyz, tetv, x):
    """|smallest barycentric coordinate| * 6 volume of x in every tetra (locate_pmmg.c's closest search), binary64"""
    p = xyz[tetv - 1]
    vol = np.einsum("ij,ij->i", p[:, 1] - p[:, 0], np.cross(p[:, 2] - p[:, 0], p[:, 3] - p[:, 0]))
    b = []
    for f in range(4):
        a, bb, c = (p[:, i] for i in IDIR[f])
        b.append(-np.einsum("ij,ij->i", x - a, np.cross(bb - a, c - a)) / vol)
    return np.abs(np.min(b, axis=0)) * vol


def _cell(k, n):
    g = int(np.ceil(n ** (1.0 / 3.0)))
    return SPACING * np.array([k % g, (k // g) % g, k // (g * g)], np.float64)


J6 = np.array([1.0, 1.0, 1.0, 1.0, 1.0, 1.0])
I6 = np.array([1.0, 0.0, 0.0, 1.0, 0.0, 1.0])
RANK1 = np.array([1.0, 2.0, 3.0, 4.0, 6.0, 9.0])  # (1, 2, 3) (1, 2, 3)^T: off-diagonals above MMG5_EPS, det exactly 0


@functools.lru_cache(maxsize=None)
def soup(seed=21):
    """The unit frame's inputs, read-only: dict(xyz, tetv, triv, sol {name: [np,
    size]}, tet_kind, tet_class, tri_class, q [nq, 3], pclass, own (1-based
    element of its class), label, src (a vertex of the own element), far (a vertex
    of another element of the class), fail {name: query indices}).

    Tetra 0..N_TET-1 and trias 0..N_TRI-1 cycle through the shapes and the tensor
    classes (met6 takes class k, ten6 class k + 1, so both see every class on
    every shape).  The last four tetra and the last two trias are the failure
    routes of invmat_failure_case, in elements with binary coordinates so that
    the coordinates (1/2, 1/2, 0[, 0]) are exact in frames 0 and 2:
      a vertex tensor RANK1 (the inversion of a vertex fails: 4 vertices, 3
      vertices, and the edge rule's 2), and the edge with the tensors 0.5 J - I
      and I at whose midpoint the interpolated inverse 0.5 J is singular."""
    rng = np.random.default_rng(seed)
    nel = N_TET + N_TRI
    xyz, tetv, triv, tet_kind, tet_class, tri_class = [], [], [], [], [], []
    sol = {name: [] for name in SIZE}
    ncls = len(TENSOR_CLASSES)

    def add_vertices(p, cls6, clsT):
        first = len(xyz) + 1
        xyz.extend(p)
        nv = len(p)
        sol["met6"].extend(_tensor_rows(rng, cls6, nv))
        sol["ten6"].extend(_tensor_rows(rng, clsT, nv))
        sol["met1"].extend(rng.uniform(0.05, 0.5, (nv, 1)))
        sol["s0"].extend([[AFFINE[0] + float(np.dot(AFFINE[1:], r))] for r in p])
        sol["s1"].extend(rng.normal(size=(nv, 1)))
        sol["s2"].extend(1e3 * rng.normal(size=(nv, 1)))
        sol["s3"].extend(-1e-3 * np.abs(rng.normal(size=(nv, 1))))
        sol["s4"].extend(rng.choice([-1.0, 1.0], (nv, 1)) * rng.uniform(0.9, 1.1, (nv, 1)))
        sol["vec"].extend(rng.normal(size=(nv, 3)))
        return list(range(first, first + nv))

    q, pclass, own, label, src, far, outside = [], [], [], [], [], [], []
    fail = dict(tet_vertex=[], tet_mint=[], tri_vertex=[], tri_edge_vertex=[], tri_mint=[])
    unit = np.array([[0, 0, 0], [0.25, 0, 0], [0, 0.25, 0], [0, 0, 0.25]], np.float64)
    for k in range(N_TET):
        special = k - (N_TET - 4)
        if special >= 0:
            p, kind = unit.copy(), "binary"
        else:
            p, kind = _tet_shape(rng, k)
        p = p + _cell(k, nel)
        c6 = (k + k // 6) % ncls  # (the shapes cycle with k % 6: every class meets every shape)
        ids = add_vertices(p, TENSOR_CLASSES[c6], TENSOR_CLASSES[(c6 + 1) % ncls])
        tetv.append(ids)
        tet_kind.append(kind)
        tet_class.append((TENSOR_CLASSES[c6], TENSOR_CLASSES[(c6 + 1) % ncls]))
        if special >= 0:
            for name in TENSOR:
                rows = sol[name]
                if special in (0, 1):
                    rows[ids[special] - 1] = RANK1
                else:
                    a, b = ((0, 1), (2, 3))[special - 2]
                    for i in range(4):
                        rows[ids[i] - 1] = I6 * (2.0 + i)
                    rows[ids[a] - 1], rows[ids[b] - 1] = 0.5 * J6 - I6, I6
            if special in (0, 1):
                phis, key = [rng.dirichlet(np.ones(4)) for _ in range(2)], "tet_vertex"
            else:
                ph = np.zeros(4)
                ph[[a, b]] = 0.5
                phis, key = [ph], "tet_mint"
            for ph in phis:
                fail[key].append(len(q))
                q.append(ph @ p if key == "tet_vertex" else 0.5 * (p[a] + p[b]))
                pclass.append(1), own.append(k + 1), label.append("fail"), src.append(ids[k % 4])
            continue
        for j, lab in enumerate(TET_QUERY):
            for _ in range(2000):
                ph = rng.dirichlet(np.ones(4))
                i = int(rng.integers(4))
                if lab.startswith("c"):
                    c = dict([("c-5e-7", -5e-7), ("c0", 0.0), ("c+5e-7", 5e-7), ("c1e-3", 1e-3)])[lab]
                    rest = np.delete(ph, i)
                    ph[np.arange(4) != i] = rest / rest.sum() * (1.0 - c)
                    ph[i] = c
                elif lab == "edge":
                    a, b = H.IARE[int(rng.integers(6))]
                    t = rng.uniform(0.1, 0.9)
                    ph = np.zeros(4)
                    ph[a], ph[b] = t, 1.0 - t
                elif lab == "vertex":
                    ph = np.zeros(4)
                    ph[i] = 1.0
                # drawn again while its smallest coordinate, as some frame rounds it, is near -MMG5_EPS
                if not any(-1.5e-6 < m < -0.7e-6 for m in _phimin_frames(p, ph @ p)) and \
                        not _near_switch(sol, ids, ph, (tet_class[-1][0] != "shortcut-mint", tet_class[-1][1] != "shortcut-mint")):
                    break
            else:
                raise AssertionError("no admissible query found")
            q.append(ph @ p)
            pclass.append(1), own.append(k + 1), label.append(lab), src.append(ids[(k + j) % 4])
        if kind in ("regular", "normal"):
            outside.append((k, p, ids))
    tets = np.array(tetv, np.int32)
    for k, p, ids in outside:
        # outside: the smallest coordinate -0.05, the others inside.  Kept where the reference's closest search (the
        # smallest |min coordinate| * volume, which is a distance times a face's area: the soup's slivers compete
        # from afar) prefers the point's own tetra by a margin of 10 %, far above the rounding of either side
        if label.count("outside") == N_OUTSIDE:
            break
        for _ in range(20):
            ph = rng.dirichlet(np.ones(4) * 3.0)
            j = int(np.argmin(ph))
            rest = np.delete(ph, j)
            ph[np.arange(4) != j] = rest / rest.sum() * 1.05
            ph[j] = -0.05
            val = _closest_values(np.array(xyz), tets, ph @ p)
            if 1.1 * val[k] < np.delete(val, k).min():
                q.append(ph @ p)
                pclass.append(1), own.append(k + 1), label.append("outside"), src.append(ids[0])
                break
    assert label.count("outside") == N_OUTSIDE
    nvol = len(q)
    flat = np.array([[0, 0, 0], [1.0, 0, 0], [0, 1.0, 0]], np.float64)
    for k in range(N_TRI):
        special = k - (N_TRI - 2)
        if special >= 0:
            p = flat.copy()
        else:  # a jittered regular tria with edges near 1: in frame 1 its coordinates resolve 1e-9 of an altitude
            ang = rng.uniform(0, 2 * np.pi) + np.array([0.0, 2.0, 4.0]) * np.pi / 3.0
            p = np.stack([np.cos(ang), np.sin(ang), np.zeros(3)], 1) * 0.58 + rng.normal(scale=0.05, size=(3, 3))
            p = p @ H._rotation(rng).T
        p = p + _cell(N_TET + k, nel)
        ids = add_vertices(p, TENSOR_CLASSES[k % ncls], TENSOR_CLASSES[(k + 1) % ncls])
        triv.append(ids)
        tri_class.append((TENSOR_CLASSES[k % ncls], TENSOR_CLASSES[(k + 1) % ncls]))
        n = np.cross(p[1] - p[0], p[2] - p[0])
        n /= np.linalg.norm(n)
        if special >= 0:
            for name in TENSOR:
                rows = sol[name]
                if special == 0:
                    rows[ids[0] - 1] = RANK1
                else:
                    rows[ids[0] - 1], rows[ids[1] - 1], rows[ids[2] - 1] = 3.0 * I6, 0.5 * J6 - I6, I6
            if special == 0:  # a face hit (3 vertices) and an edge hit whose edge ends at the vertex
                for ph, key in ((np.array([0.25, 0.5, 0.25]), "tri_vertex"), (np.array([0.5, 0.5, 0.0]), "tri_edge_vertex")):
                    fail[key].append(len(q))
                    q.append(ph @ p)
                    pclass.append(2), own.append(k + 1), label.append("fail"), src.append(ids[1])
            else:  # the midpoint of edge 0 (vertices 1 and 2): both rules' interpolated inverse is 0.5 J
                fail["tri_mint"].append(len(q))
                q.append(0.5 * (p[1] + p[2]))
                pclass.append(2), own.append(k + 1), label.append("fail"), src.append(ids[2])
            continue
        for j, lab in enumerate(TRI_QUERY):
            tiny = lambda: rng.choice([0.0, 1e-9, -1e-9, 3e-10])
            for _ in range(2000):  # (drawn again while an interpolated inverse's off-diagonals come near the switch)
                ph = rng.dirichlet(np.ones(3) * 2.0)
                ph = np.maximum(ph, 0.02)
                ph /= ph.sum()
                i = int(rng.integers(3))
                if lab == "edge":
                    t = rng.uniform(0.1, 0.9)
                    ph = np.array([t, 1.0 - t, 0.0])[np.roll(np.arange(3), i)]
                    ph[ph == 0.0] = tiny()
                elif lab == "vertex":
                    ph = np.array([tiny(), tiny(), 0.0])
                    ph[2] = 1.0 - ph[0] - ph[1]
                    ph = ph[np.roll(np.arange(3), i)]
                big = int(np.argmax(ph))
                ph[big] = 1.0 - np.delete(ph, big).sum()  # (a sum off by 1e-9 moves the point by 1e-9 of its position)
                if not _near_switch(sol, ids, ph, (tri_class[-1][0] != "shortcut-mint", tri_class[-1][1] != "shortcut-mint")):
                    break
            else:
                raise AssertionError("no admissible query found")
            d = 0.0 if (k + j) % 5 == 0 else rng.choice([-1.0, 1.0]) * rng.uniform(0.05, 0.45) * HAUSD
            q.append(ph @ p + d * n)
            pclass.append(2), own.append(k + 1), label.append(lab), src.append(ids[(k + j) % 3])
    tetv, triv = np.array(tetv, np.int32), np.array(triv, np.int32)
    own, pclass = np.array(own, np.int32), np.array(pclass, np.uint8)
    for i in range(len(q)):  # a vertex of the next element of the same class: a walk from there ends at once
        conn = tetv if pclass[i] == 1 else triv
        far.append(int(conn[own[i] % conn.shape[0]][0]))
    out = dict(xyz=np.array(xyz), tetv=tetv, triv=triv, sol={k: np.array(v, np.float64) for k, v in sol.items()},
               tet_kind=tuple(tet_kind), tet_class=tuple(tet_class), tri_class=tuple(tri_class), q=np.array(q),
               pclass=pclass, own=own, label=tuple(label), src=np.array(src, np.int32), far=np.array(far, np.int32),
               fail={k: tuple(v) for k, v in fail.items()}, nvol=nvol)
    assert out["q"].shape[0] <= 2000
    for a in [out["xyz"], tetv, triv, out["q"], pclass, own, out["src"], out["far"]] + list(out["sol"].values()):
        a.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def frame_inputs(fi):
    """(xyz, q, hausd) of the soup in FRAMES[fi], read-only"""
    s, t = FRAMES[fi]
    S = soup()
    xyz, q = np.ascontiguousarray(S["xyz"] * s + t), np.ascontiguousarray(S["q"] * s + t)
    xyz.setflags(write=False)
    q.setflags(write=False)
    return xyz, q, HAUSD * s


def background(fi, met=None, fields=()):
    """(mesh, oracle background) of the soup in FRAMES[fi] with the named solutions"""
    from oracle import oracle as O
    from parmmg_amd.synth import CUBE, Mesh
    S = soup()
    xyz, _, hausd = frame_inputs(fi)
    mesh = Mesh(CUBE, 0, xyz, S["tetv"], np.zeros((S["tetv"].shape[0], 4), np.int32), S["triv"],
                np.zeros((S["triv"].shape[0], 3), np.int32), None)
    return mesh, O.Background(mesh, None if met is None else S["sol"][met], [S["sol"][f] for f in fields], hausd)


@functools.lru_cache(maxsize=None)
def vertex_inverses(name):
    """invmat of every vertex tensor of solution `name` (the same in every frame)"""
    return tuple(invmat(_v(r)) for r in soup()["sol"][name])


def rows_over(ids, phi, dphi):
    """{solution: (value or None, bounds)} of the whole pool over the vertices ids
    (1-based) with the coordinates phi +- dphi; tensors also give "off:" + name,
    the interpolated inverse's largest off-diagonal"""
    S = soup()["sol"]
    out = {}
    for name in ISO:
        out[name] = interp_p1(phi, dphi, [S[name][i - 1] for i in ids])
    for name in TENSOR:
        inv = vertex_inverses(name)
        v, b, off = interp_tensor(phi, dphi, [inv[i - 1] for i in ids])
        out[name] = (v, b)
        out["off:" + name] = off
    return out


def copy_rows(i):
    """a vertex hit's metric: the vertex's row, exactly"""
    S = soup()["sol"]
    return {name: (_v(S[name][i - 1]), [ZERO] * SIZE[name]) for name in ("met1", "met6")}


@functools.lru_cache(maxsize=None)
def reference(fi):
    """The definition's values of every query of the soup in FRAMES[fi], a list of
    dicts per query.  A volume query: phi, dphi, phimin, "all" (the four vertices'
    rule: VOL_WALK, VOL_EXHAUST) and "closest" (VOL_CLOSEST: the unit coordinate on
    the nearest vertex).  A surface query: phi, dphi, dist, ddist, kind and loc
    (PMMG_barycoord_isBorder), "all" (the three vertices for every solution:
    BDY_EXHAUST, and every field of any hit) and "met" (the metric's rows under
    kind: a copy, the edge's two ends, or the face).  Rows are {solution: (value
    or None where the row stays untouched, bounds)} as rows_over gives them."""
    S = soup()
    xyz, q, _ = frame_inputs(fi)
    out = []
    for i in range(q.shape[0]):
        if S["pclass"][i] == 1:
            ids = [int(t) for t in S["tetv"][S["own"][i] - 1]]
            p = xyz[np.array(ids) - 1]
            phi, dphi = tet_coords(p, q[i])
            out.append(dict(phi=phi, dphi=dphi, phimin=min(phi), all=rows_over(ids, phi, dphi),
                            closest=rows_over(ids, nearest_vertex(p, q[i]), [ZERO] * 4)))
        else:
            ids = [int(t) for t in S["triv"][S["own"][i] - 1]]
            phi, dphi, dist, ddist = tria_coords(xyz[np.array(ids) - 1], q[i])
            kind, loc = border(phi)
            r = dict(phi=phi, dphi=dphi, phimin=min(phi), dist=dist, ddist=ddist, kind=kind, loc=loc,
                     all=rows_over(ids, phi, dphi))
            if kind == BDY_VERTEX:
                r["met"] = copy_rows(ids[loc])
            elif kind == BDY_EDGE:
                e = edge_ends(loc)
                sub = rows_over([ids[j] for j in e], [phi[j] for j in e], [dphi[j] for j in e])
                r["met"] = {k: v for k, v in sub.items() if k.endswith(("met1", "met6"))}
            else:
                r["met"] = r["all"]
            out.append(r)
    return out


def rule_rows(ref, hit, metric):
    """the rows the definition gives a query under the hit kind the device
    reported (interpmesh_pmmg.c:563-636): {solution: (value, bounds)}; metric: the
    solution that stands in the metric's place (None: no metric)"""
    if hit in (VOL_WALK, VOL_EXHAUST):
        return ref["all"]
    if hit == VOL_CLOSEST:
        return ref["closest"]
    if hit == BDY_EXHAUST or metric is None:
        return ref["all"]
    assert hit == ref["kind"], (hit, ref["kind"])
    return dict(ref["all"], **{metric: ref["met"][metric]})


def row_ratio(got, value, bound):
    """(worst |got - value| / bound over a row's components, tight): got binary64,
    taken exactly; tight: every bound below 1e-9 of the row's largest modulus"""
    worst = 0.0
    for g, v, b in zip(got, value, bound):
        err = abs(mp.mpf(float(g)) - v)
        r = float(err / b) if b > 0 else (0.0 if err == 0 else float("inf"))
        worst = max(worst, r) if r == r else float("inf")
    big = max(abs(v) for v in value)
    return worst, bool(max(bound) < mp.mpf(1e-9) * big)
