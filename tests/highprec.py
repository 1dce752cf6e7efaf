"""The quality and weight operations in 50-digit arithmetic, with forward
error bounds for their binary64 evaluation, and the seeded inputs the CPU and
GPU tests share (tests/test_highprec_host.py, test_gpu_quality.py,
test_gpu_wgt.py).

Every function is written from the mathematical definition (a determinant, a
quadratic form v^T M v, a logarithm), not in the operation order of
oracle/pmmg_oracle.c or pmmg_quality.hip, and takes its inputs as the exact
binary64 values (mp.mpf(float(x))).  It returns (value, bound): bound is what a
binary64 evaluation of the same formula may be off by, built from the
computation's own condition with u = 2^-53.  The bounds are the condition the
CPU oracle satisfies on the committed inputs (test_highprec_host.py); the
device is then held to the same bounds.  No constant here is fitted to any
output: each docstring gives the operation count it comes from.

The tables are written out again from Mmg's definition (libmmgtypes: MMG5_iare
[i] = the two vertices of edge i; MMG5_iarf[f] = the three edges of face f, the
face opposite vertex f), and checked against that definition below."""
from __future__ import annotations

import functools

import numpy as np
from mpmath import mp

mp.dps = 50
U = mp.mpf(2) ** -53
EPSD2 = mp.mpf(1.0e-200)
EPSOK = mp.mpf(1.0e-20)
MMG_EPS = mp.mpf(1.0e-06)
HUGE = mp.mpf(1000000)

IARE = ((0, 1), (0, 2), (0, 3), (1, 2), (1, 3), (2, 3))
IARF = ((5, 4, 3), (5, 1, 2), (4, 2, 0), (3, 0, 1))
for _f in range(4):  # a face's edges are the three that do not touch the vertex opposite
    assert sorted(IARF[_f]) == [e for e in range(6) if _f not in IARE[e]]


def _v(x):
    return [mp.mpf(float(t)) for t in x]


def _sub(a, b):
    return [y - x for x, y in zip(a, b)]


def _perm(ab, ac, ad):
    """the six products of the 3 x 3 determinant, every one made absolute"""
    a, b, c = [[abs(t) for t in r] for r in (ab, ac, ad)]
    return (a[0] * (b[1] * c[2] + b[2] * c[1]) + a[1] * (b[2] * c[0] + b[0] * c[2]) + a[2] * (b[0] * c[1] + b[1] * c[0]))


def _edges(p):
    return [_sub(p[i], p[j]) for i, j in IARE]


def _quad(m, v, absolute=False):
    """v^T M v for M = (m11 m12 m13 m22 m23 m33); absolute: every term's modulus"""
    M = ((m[0], m[1], m[2]), (m[1], m[3], m[4]), (m[2], m[4], m[5]))
    terms = [M[i][j] * v[i] * v[j] for i in range(3) for j in range(3)]
    return sum(abs(t) for t in terms) if absolute else sum(terms)


def qual_iso(p):
    """MMG5_caltet_iso: q = vol / rap^1.5, vol = det(b - a, c - a, d - a), rap the
    sum of the six squared edge lengths; 0 for vol < MMG5_EPSD2.

    Bound u (8 perm / rap^1.5 + 12 q).  Each of the six products of the
    determinant carries 3 rounded differences, 2 multiplications and at most 3
    additions: 8 u perm on vol.  rap is a sum of squares (no cancellation): 2
    (differences) + 1 (square) + at most 3 more roundings on the way through the
    sums give it a relative error below 6 u, 1.5 times that on rap^1.5, plus the
    square root, the product and the quotient: 12 u q in all.  Where vol <
    EPSD2 the value is 0 and the first term alone stands for a computed vol that
    came out above the threshold."""
    p = [_v(x) for x in p]
    ab, ac, ad = _sub(p[0], p[1]), _sub(p[0], p[2]), _sub(p[0], p[3])
    vol = mp.det(mp.matrix([ab, ac, ad]))
    rap = sum(t * t for e in _edges(p) for t in e)
    r15 = rap * mp.sqrt(rap)
    q = vol / r15 if vol >= EPSD2 else mp.mpf(0)
    return q, U * (8 * _perm(ab, ac, ad) / r15 + 12 * q)


def qual_ani(p, rows):
    """MMG5_caltet_ani: q = sqrt(det M) vol / rap_M^1.5 with M the average of
    the four vertex tensors rows[4][6] and rap_M the sum of e^T M e over the six
    edges; 0 for vol <= 0 or det M < MMG5_EPSOK.

    Bound u q (8 perm / |vol| + 3 det_abs / det + 15 rap_abs / rap + 12) plus the
    average's own error.  8 perm as in qual_iso.  det M: three factors, 2
    multiplications and at most 3 additions per product, 6 u det_abs, halved by
    the square root.  rap_M: per term 2 differences, 3 multiplications (the
    factor 2 is exact) and at most 5 additions within and across the six forms,
    10 u rap_abs, times 1.5.  12 as in qual_iso.  The average is three additions
    and an exact scaling by 1/4: each component of M is off by at most 4 u
    mean|row| (3 rounded up), which moves det by sum |d det / d m_j| dm_j and
    rap_M by the forms evaluated with |e| and dm.  Written with q multiplied in,
    so that a vanishing vol divides nothing."""
    p = [_v(x) for x in p]
    rows = [_v(r) for r in rows]
    m = [sum(r[j] for r in rows) / 4 for j in range(6)]
    dm = [4 * U * sum(abs(r[j]) for r in rows) / 4 for j in range(6)]
    ab, ac, ad = _sub(p[0], p[1]), _sub(p[0], p[2]), _sub(p[0], p[3])
    vol = mp.det(mp.matrix([ab, ac, ad]))
    M = mp.matrix([[m[0], m[1], m[2]], [m[1], m[3], m[4]], [m[2], m[4], m[5]]])
    det = mp.det(M)
    a = [abs(t) for t in m]
    det_abs = (a[0] * a[3] * a[5] + 2 * a[1] * a[2] * a[4] + a[0] * a[4] * a[4] + a[3] * a[2] * a[2] + a[5] * a[1] * a[1])
    ddet = (dm[0] * (a[3] * a[5] + a[4] * a[4]) + dm[3] * (a[0] * a[5] + a[2] * a[2]) + dm[5] * (a[0] * a[3] + a[1] * a[1]) +
            2 * dm[1] * (a[2] * a[4] + a[1] * a[5]) + 2 * dm[2] * (a[1] * a[4] + a[2] * a[3]) +
            2 * dm[4] * (a[1] * a[2] + a[0] * a[4]))
    E = _edges(p)
    rap = sum(_quad(m, e) for e in E)
    rap_abs = sum(_quad(m, e, True) for e in E)
    drap = sum(_quad(dm, [abs(t) for t in e], True) for e in E)
    if not (det >= EPSOK and rap > 0):
        return mp.mpf(0), mp.inf  # (not a case of the high-precision tests: the branch fixtures cover it)
    sd = mp.sqrt(det)
    r15 = rap * mp.sqrt(rap)
    q = sd * vol / r15 if vol > 0 else mp.mpf(0)
    bound = U * (8 * _perm(ab, ac, ad) * sd / r15 + q * (3 * det_abs / det + 15 * rap_abs / rap + 12))
    bound += q * (ddet / (2 * det) + 3 * drap / (2 * rap))
    return q, bound


def len_iso(a, b, h1, h2):
    """MMG5_lenedgCoor_iso: with l = |b - a| and r = h2 / h1 - 1, l / h1 for
    |r| < MMG5_EPS, else l ln(h2 / h1) / (h2 - h1).

    l: 1 (difference) + 0.5 (square) per term, 2 additions and half of it all
    through the root, 1 more for the root: below 4 u.  First branch: one
    division more, 6 u relative with a margin of one.  Second: the division, h2
    - h1, the product, and a log1p of up to 1 ulp as ROCm documents it: 8 u; and
    the argument r = fl(h2 / h1) - 1 carries the quotient's rounding u (h2 / h1)
    (the subtraction is exact or rounds once more), which the logarithm turns
    into a relative 2 u (h2 / h1) / |r| at most (ln(1 + r) ~ r near the switch,
    where this reaches about 1e-10: the reference's own arithmetic)."""
    a, b, h1, h2 = _v(a), _v(b), mp.mpf(float(h1)), mp.mpf(float(h2))
    l = mp.sqrt(sum(t * t for t in _sub(a, b)))
    r = h2 / h1 - 1
    if abs(r) < MMG_EPS:
        v = l / h1
        return v, 6 * U * v
    v = l * mp.log(h2 / h1) / (h2 - h1)
    return v, U * (8 + 2 * (h2 / h1) / abs(r)) * v


def _dsqrt(x, e):
    """how far sqrt moves when its non-negative argument x moves by e (clamped
    at 0): e / sqrt(x) from the mean value, sqrt(e) from concavity, whichever
    is smaller"""
    if x <= 0:
        return mp.sqrt(e)
    return min(e / mp.sqrt(x), mp.sqrt(e))


def len_ani(a, b, sa, sb):
    """MMG5_lenedgCoor_ani without ridge storage: dd_i = max(e^T S_i e, 0) at
    both ends, the midpoint value sqrt((dd1 + dd2) / 2) for |dd1 - dd2| < 0.05,
    else Simpson's (sqrt dd1 + sqrt dd2 + 4 sqrt((dd1 + dd2) / 2)) / 6.
    Returns (value, bound, ambiguous).

    Each form: per term 2 rounded differences, 2 multiplications and 2 to 3
    additions: 6 u dd_abs (dd_abs the sum of the terms' moduli; the clamp is
    continuous and adds nothing).  The strict first-order count is 7 for the
    four terms that pass three additions and 6 for the other two; the smaller
    figure is kept, as the tighter check (the worst ratio measured is 0.21).  mid = (dd1 + dd2) / 2 is off by e1 / 2 + e2 /
    2 + u mid.  A root moves by _dsqrt of its argument's error, plus u of its
    own.  Midpoint branch: that is all.  Simpson: the three roots' errors
    weighted 1, 1, 4, two additions and the exact factor 4, the division: 3 u of
    the (all positive) sum more, over 6.  ambiguous: |dd1 - dd2| is within e1 +
    e2 + u |dd1 - dd2| of 0.05, so the binary64 evaluation may take either
    branch."""
    a, b, sa, sb = _v(a), _v(b), _v(sa), _v(sb)
    e = _sub(a, b)
    dd, err = [], []
    for s in (sa, sb):
        d = _quad(s, e)
        err.append(6 * U * _quad(s, e, True))
        dd.append(d if d > 0 else mp.mpf(0))
    gap = abs(dd[0] - dd[1])
    ambiguous = abs(gap - mp.mpf(0.05)) <= err[0] + err[1] + U * gap
    mid = (dd[0] + dd[1]) / 2
    emid = (err[0] + err[1]) / 2 + U * mid
    smid, dmid = mp.sqrt(mid), _dsqrt(mid, emid) + U * mp.sqrt(mid)
    if gap < mp.mpf(0.05):
        return smid, dmid, ambiguous
    s1, s2 = mp.sqrt(dd[0]), mp.sqrt(dd[1])
    v = (s1 + s2 + 4 * smid) / 6
    bound = (_dsqrt(dd[0], err[0]) + U * s1 + _dsqrt(dd[1], err[1]) + U * s2 + 4 * dmid) / 6 + 3 * U * v
    return v, bound, ambiguous


def face_edges(v, ifac, iarf=IARF):
    """the (ip1, ip2) vertex pairs (1-based ids of v) of face ifac's three edges"""
    return [(int(v[IARE[ia][0]]), int(v[IARE[ia][1]])) for ia in iarf[ifac]]


def face_wgt(xyz, v, ifac, met, iarf=IARF, rate=(28, 3), simpson=4):
    """PMMG_computeWgt: w = min(exp(-28 res / 3), PMMG_WGTVAL_HUGEINT), res the sum
    over the face's three edges of len - 1 (len <= 1) or 1 / len - 1 (len > 1), len
    the edge's length in the metric met ([np, 1] sizes or [np, 6] tensors).
    Returns (value, bound, ambiguous edges).

    Bound w (28/3 dres + u (4 + |28 res / 3|)).  dres is the sum of the edges'
    bounds: the length's bound (over len^2 past 1: d(1/len)), u / len for the
    reciprocal, and 3 u |term| for the subtraction and the two additions the
    term then passes through (len - 1 is exact near 1).  The argument's two
    roundings and an exp of up to 1 ulp, as ROCm documents it, and the
    reciprocal: u (4 + |28 res / 3|).  The term is continuous at len = 1 and the
    cap is continuous in w, so neither switch adds a case; a weight that stays
    above the cap by more than its bound is the cap exactly.

    iarf, rate, simpson: the altered variants of the harness self-check
    (test_highprec_host.py); the defaults are the operation."""
    met = np.asarray(met)
    res, dres, amb = mp.mpf(0), mp.mpf(0), 0
    for ip1, ip2 in face_edges(v, ifac, iarf):
        ca, cb = xyz[ip1 - 1], xyz[ip2 - 1]
        if met.shape[1] == 1:
            ln, dl = len_iso(ca, cb, met[ip1 - 1, 0], met[ip2 - 1, 0])
        elif simpson == 4:
            ln, dl, a = len_ani(ca, cb, met[ip1 - 1], met[ip2 - 1])
            amb += int(a)
        else:
            ln, dl = _len_ani_altered(ca, cb, met[ip1 - 1], met[ip2 - 1], simpson)
        if ln <= 1:
            term, dt = ln - 1, dl
        else:
            term, dt = 1 / ln - 1, dl / (ln * ln) + U / ln
        res += term
        dres += dt + 3 * U * abs(term)
    x = mp.mpf(rate[0]) * res / rate[1]
    w = mp.exp(-x)
    bound = w * (mp.mpf(rate[0]) / rate[1] * dres + U * (4 + abs(x)))
    if w - bound >= HUGE:
        return HUGE, mp.mpf(0), amb
    return min(w, HUGE), bound, amb


def _len_ani_altered(a, b, sa, sb, weight):
    """len_ani's Simpson branch with another weight on the midpoint (self-check only)"""
    a, b, sa, sb = _v(a), _v(b), _v(sa), _v(sb)
    e = _sub(a, b)
    dd = [max(_quad(s, e), mp.mpf(0)) for s in (sa, sb)]
    mid = (dd[0] + dd[1]) / 2
    if abs(dd[0] - dd[1]) < mp.mpf(0.05):
        return mp.sqrt(mid), mp.mpf(0)
    return (mp.sqrt(dd[0]) + mp.sqrt(dd[1]) + weight * mp.sqrt(mid)) / (2 + weight), mp.mpf(0)


# ---------------------------------------------------------------- shared inputs
#
# Every tetra of these inputs has four vertices of its own (tetv = 1..4n in
# rows), so a case is one row of each array and nothing is shared.

REG = np.array([[1, 1, 1], [-1, 1, -1], [1, -1, -1], [-1, -1, 1]], np.float64)  # positively oriented
FRAMES = tuple((s, t) for s in (1.0, 1e-4, 1e3) for t in (0.0, 1e3))  # x -> s x + t


def _orient(p):
    return p if np.linalg.det(p[1:] - p[0]) > 0 else p[[0, 2, 1, 3]]


def _rotation(rng):
    q, r = np.linalg.qr(rng.normal(size=(3, 3)))
    return q * np.sign(np.diag(r))


def sym6(M):
    return np.array([M[0, 0], M[0, 1], M[0, 2], M[1, 1], M[1, 2], M[2, 2]])


def tensor(rng, lo, hi):
    """Q diag(lam) Q^T with lam log-uniform over [lo, hi], as (Q, lam)"""
    return _rotation(rng), np.exp(rng.uniform(np.log(lo), np.log(hi), 3))


def _sliver(rng, h):
    """a tetra whose fourth vertex stands h times the base's size above a point inside the base"""
    base = rng.normal(size=(3, 3))
    n = np.cross(base[1] - base[0], base[2] - base[0])
    size = np.sqrt(np.linalg.norm(n))
    w = rng.dirichlet((2.0, 2.0, 2.0))
    return _orient(np.vstack([base, w @ base + h * size * n / np.linalg.norm(n)]))


@functools.lru_cache(maxsize=None)
def qual_geometry(seed=11):
    """([4 n, 3] xyz, [n, 4] tetv, labels): regular, random normal and sliver
    tetra (relative height 1e-3, 1e-7, 1e-9) in the six FRAMES.  The 1e-9
    slivers keep the unshifted frames: past a shift of 1e3 their height is
    below the coordinates' spacing and the rounded input is no sliver of that
    height any more."""
    rng = np.random.default_rng(seed)
    base, lab = [], []
    for _ in range(10):
        base.append(_orient((REG * rng.uniform(0.5, 2.0)) @ _rotation(rng).T + rng.normal(size=3)))
        lab.append("regular")
    for _ in range(200):
        base.append(_orient(rng.normal(size=(4, 3))))
        lab.append("normal")
    for h in (1e-3, 1e-7, 1e-9):
        for _ in range(40):
            base.append(_sliver(rng, h))
            lab.append("sliver%.0e" % h)
    pts, labels = [], []
    for s, t in FRAMES:
        for p, name in zip(base, lab):
            if name == "sliver1e-09" and t != 0.0:
                continue
            pts.append(p * s + t)
            labels.append(name)
    xyz = np.ascontiguousarray(np.vstack(pts))
    tetv = np.arange(1, xyz.shape[0] + 1, dtype=np.int32).reshape(-1, 4)
    xyz.setflags(write=False)
    tetv.setflags(write=False)
    return xyz, tetv, tuple(labels)


@functools.lru_cache(maxsize=None)
def qual_tensors(seed=12):
    """[4 n, 6] vertex tensors for qual_geometry: Q diag(lam) Q^T per tetra, lam
    over 1e-4..1e4 (two in three) or 1e-6..1e2, each of the four rows with its
    eigenvalues moved by up to 10 % (so the average is one of four different,
    still definite rows)."""
    rng = np.random.default_rng(seed)
    n = qual_geometry()[1].shape[0]
    met = np.empty((4 * n, 6))
    for k in range(n):
        Q, lam = tensor(rng, *((1e-6, 1e2) if k % 3 == 2 else (1e-4, 1e4)))
        for i in range(4):
            met[4 * k + i] = sym6((Q * (lam * (1.0 + rng.uniform(-0.1, 0.1, 3)))) @ Q.T)
    met.setflags(write=False)
    return met


@functools.lru_cache(maxsize=None)
def qual_reference(ani):
    """([n] values, [n] bounds) of qual_geometry in mpmath, as Python lists of mpf"""
    xyz, tetv, _ = qual_geometry()
    met = qual_tensors() if ani else None
    out = [qual_ani(xyz[v - 1], met[v - 1]) if ani else qual_iso(xyz[v - 1]) for v in tetv]
    return [o[0] for o in out], [o[1] for o in out]


R_SWITCH = (1e-7, 0.9e-6, 1.1e-6, 1e-5, 1e-3)  # |h2 / h1 - 1| around MMG5_EPS = 1e-6


def _unit_tetra(rng):
    """a jittered regular tetra with edges near 1"""
    p = (REG / np.sqrt(8.0)) @ _rotation(rng).T + rng.normal(scale=0.07, size=(4, 3)) + rng.normal(size=3)
    return _orient(p)


def iso_r(met, v):
    """the six r = h2 / h1 - 1 of a tetra's edges, as the kernel forms them"""
    return np.array([met[v[j] - 1, 0] / met[v[i] - 1, 0] - 1.0 for i, j in IARE])


@functools.lru_cache(maxsize=None)
def wgt_iso_inputs(seed=13, n=420):
    """(xyz, tetv, met [4 n, 1]): unit-ish tetra; one in three with sizes
    uniform over 0.3..1.5, the others with the sizes of vertices 1..3 at h0 (1 +-
    r), r from R_SWITCH.  A tetra with an edge whose |r| falls between 0.9e-6 and
    1.1e-6 is drawn again: nothing sits between."""
    rng = np.random.default_rng(seed)
    xyz, met = np.empty((4 * n, 3)), np.empty((4 * n, 1))
    tetv = np.arange(1, 4 * n + 1, dtype=np.int32).reshape(-1, 4)
    for k in range(n):
        xyz[4 * k:4 * k + 4] = _unit_tetra(rng)
        while True:
            if k % 3 == 0:
                h = rng.uniform(0.3, 1.5, 4)
            else:
                h0 = rng.uniform(0.3, 1.5)
                h = h0 * (1.0 + np.concatenate([[0.0], rng.choice(R_SWITCH, 3) * rng.choice([-1.0, 1.0], 3)]))
            met[4 * k:4 * k + 4, 0] = h
            r = np.abs(iso_r(met, tetv[k]))
            if not ((r > 0.9e-6) & (r < 1.1e-6)).any():
                break
    for a in (xyz, tetv, met):
        a.setflags(write=False)
    return xyz, tetv, met


def ani_gaps(xyz, met, v):
    """|dd1 - dd2| of a tetra's six edges in binary64 (dd clamped at 0)"""
    out = []
    for i, j in IARE:
        e = xyz[v[j] - 1] - xyz[v[i] - 1]
        dd = []
        for s in (met[v[i] - 1], met[v[j] - 1]):
            M = np.array([[s[0], s[1], s[2]], [s[1], s[3], s[4]], [s[2], s[4], s[5]]])
            dd.append(max(float(e @ M @ e), 0.0))
        out.append(abs(dd[0] - dd[1]))
    return np.array(out)


@functools.lru_cache(maxsize=None)
def wgt_ani_inputs(seed=14, n=420):
    """(xyz, tetv, met [4 n, 6]): unit-ish tetra under Q diag(lam) Q^T with lam
    over 0.1..10 (lengths on both sides of 1, weights below and at the cap); the
    four rows' eigenvalues differ by up to 1 % (even k: |dd1 - dd2| small, the
    midpoint branch) or up to 50 % (odd k: Simpson).  A tetra with an edge whose
    |dd1 - dd2| falls between 0.049 and 0.051 is drawn again."""
    rng = np.random.default_rng(seed)
    xyz, met = np.empty((4 * n, 3)), np.empty((4 * n, 6))
    tetv = np.arange(1, 4 * n + 1, dtype=np.int32).reshape(-1, 4)
    for k in range(n):
        xyz[4 * k:4 * k + 4] = _unit_tetra(rng)
        spread = 0.01 if k % 2 == 0 else 0.5
        while True:
            Q, lam = tensor(rng, 0.1, 10.0)
            for i in range(4):
                met[4 * k + i] = sym6((Q * (lam * (1.0 + rng.uniform(-spread, spread, 3)))) @ Q.T)
            g = ani_gaps(xyz, met, tetv[k])
            if not ((g > 0.049) & (g < 0.051)).any():
                break
    for a in (xyz, tetv, met):
        a.setflags(write=False)
    return xyz, tetv, met


@functools.lru_cache(maxsize=None)
def wgt_reference(ani):
    """([n][4] values, bounds, ambiguous counts) of the weight inputs' faces in mpmath"""
    xyz, tetv, met = wgt_ani_inputs() if ani else wgt_iso_inputs()
    out = [[face_wgt(xyz, v, f, met) for f in range(4)] for v in tetv]
    return ([[o[0] for o in r] for r in out], [[o[1] for o in r] for r in out], [[o[2] for o in r] for r in out])


def ratios(got, values, bounds):
    """(|got - value| / bound per element, share of elements with bound < 1e-9
    |value|); got: binary64 numbers, taken exactly.  A zero error over a zero
    bound counts as 0, any error over a zero bound as inf."""
    rat, tight = [], 0
    for g, v, b in zip(got, values, bounds):
        err = abs(mp.mpf(float(g)) - v)
        rat.append(float(err / b) if b > 0 else (0.0 if err == 0 else float("inf")))
        tight += int(b < mp.mpf(1e-9) * abs(v))
    return np.array(rat), tight / max(len(rat), 1)


def flat(rows):
    return [x for r in rows for x in r]


def stretched_metric(xyz, lam=(1.0, 1e2, 1e4), seed=15):
    """[np, 6] tensors for a lattice: one rotation, eigenvalues lam / h^2 with h
    = 0.2 times a smooth factor of the position (by default a 1e4 stretch, under
    which every face weight is at the cap; lam = (0.6, 1, 1.8) keeps lengths
    near 1 and most weights below it)"""
    rng = np.random.default_rng(seed)
    Q = _rotation(rng)
    f = 1.0 + 0.3 * np.sin(3.0 * xyz[:, 0]) * np.cos(2.0 * xyz[:, 1]) + 0.2 * xyz[:, 2]
    return np.ascontiguousarray([sym6((Q * (np.array(lam) / (0.2 * s) ** 2)) @ Q.T) for s in f])


def graded_sizes(xyz, seed=16):
    """[np, 1] sizes for a lattice of spacing 0.2: 0.2 times a factor over 0.5..1.6"""
    rng = np.random.default_rng(seed)
    return np.ascontiguousarray(0.2 * rng.uniform(0.5, 1.6, (xyz.shape[0], 1)))
