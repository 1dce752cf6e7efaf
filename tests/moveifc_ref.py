"""The interface displacement of the reference restated twice in Python: what
pmmg_hip_ifc_seed / pmmg_hip_ifc_layers / pmmg_hip_remap_colors are compared
with (tests/test_gpu_moveifc.py), and what tests/test_moveifc_ref_host.py
proves equal to each other on the CPU.

  seed_seq()   PMMG_mark_interfacePoints (src/moveinterfaces_pmmg.c:1052-1090)
               with its fields: tmp, s, flag
  ifc_seq()    the layer loop of PMMG_part_moveInterfaces (:1366-1439) with
               PMMG_mark_boulevolp (:832-933) and PMMG_mark_sideFront
               (:947-1038): points in ascending id, the ball by BFS over the
               links from the point's handle s, mark / tmp / s / flag / base,
               negrp with the return in the middle of a ball.  side_tie is the
               side point's choice among tetra of equal least weight: "bfs"
               the reference's (first in BFS order), "lowest" the module's
               (lowest tetra id).  ball="star" visits the whole vertex star
               instead of its face-connected part around s.
  seed_par(), ifc_par()
               the definition of include/parmmg_hip.h ("Interface
               displacement") in array operations over all tetra: no point
               order, no traversal, the whole star
  remap()      the DISTR branch of PMMG_part_getInterfaces (:1176-1211)

Arrays are 0-based rows of 1-based entities as everywhere in the tests: tetv
[ne, 4] vertex ids (v[0] <= 0: unused tetra), adja [ne, 4] links 4 k' + f' or
0, mark [ne] colours in [0, ncolor), w [ncolor] > 0 (c beats d iff w[c] <
w[d]).  Point arrays have np entries, entry p - 1 for point p: color (-1: in
no used tetra) and front (0 / 1).  nelem [ncolor] is negrp (-1: not local,
never brakes), nemin [ncolor] its floor.
"""
import numpy as np

NELEM_MIN = 6  # PMMG_REDISTR_NELEM_MIN


def nemin_of(nelem):
    """MG_MIN(PMMG_REDISTR_NELEM_MIN, negrp / 2 + 1) per colour (0 where the colour is not local)"""
    n = np.asarray(nelem, np.int64)
    return np.where(n >= 0, np.minimum(NELEM_MIN, n // 2 + 1), 0).astype(np.int32)


def stars(tetv):
    """list over points (entry p - 1) of the used tetra (0-based, ascending) that contain p; np = the largest id"""
    tetv = np.asarray(tetv)
    out = [[] for _ in range(int(tetv.max()))]
    for k, row in enumerate(tetv.tolist()):
        if row[0] > 0:
            for v in row:
                out[v - 1].append(k)
    return out


def stars_face_connected(tetv, adja):
    """True iff the star of every point is connected through faces that contain the point: the ball the reference
    walks from any handle is then the whole star"""
    tetv, adja = np.asarray(tetv), np.asarray(adja)
    tl, al = tetv.tolist(), adja.tolist()
    for p0, star in enumerate(stars(tetv)):
        if len(star) < 2:
            continue
        p, inside = p0 + 1, set(star)
        seen, todo = {star[0]}, [star[0]]
        while todo:
            k = todo.pop()
            for f in range(4):
                if tl[k][f] == p or not al[k][f]:
                    continue  # (the face opposite p does not contain it)
                j = al[k][f] // 4 - 1
                if j in inside and j not in seen:
                    seen.add(j)
                    todo.append(j)
        if len(seen) != len(star):
            return False
    return True


# ---------------------------------------------------------------- the transcribed loop

def seed_seq(tetv, mark, w, np_):
    """dict(tmp, s, flag, bf): lists indexed by point id (entry 0 unused); s = 4 (k + 1) + iloc"""
    tmp, s, flag = [-1] * (np_ + 1), [0] * (np_ + 1), [0] * (np_ + 1)
    bf = 1
    ml, wl = np.asarray(mark).tolist(), np.asarray(w).tolist()
    for k, row in enumerate(np.asarray(tetv).tolist()):
        if row[0] <= 0:
            continue
        for iloc, p in enumerate(row):
            if tmp[p] < 0:
                tmp[p], s[p] = ml[k], 4 * (k + 1) + iloc
            elif wl[tmp[p]] > wl[ml[k]]:
                tmp[p], s[p], flag[p] = ml[k], 4 * (k + 1) + iloc, bf
    return dict(tmp=tmp, s=s, flag=flag, bf=bf)


def _ball(tl, al, star, p, start, ball):
    """the tetra around p in the order the reference lists them (0-based) from `start`"""
    if ball == "star":
        return [start] + [k for k in star if k != start]
    lst, seen, cur = [start], {start}, 0
    while cur < len(lst):
        k = lst[cur]
        i = tl[k].index(p)
        for _ in range(3):
            i = (i + 1) % 4
            if al[k][i]:
                j = al[k][i] // 4 - 1
                if j not in seen:
                    seen.add(j)
                    lst.append(j)
        cur += 1
    return lst


def ifc_seq(tetv, adja, mark, w, nelem, nemin, np_, nlayers, set_pt=None, set_color=None, side_tie="lowest",
            ball="ball", state=None):
    """list of one dict per layer (mark, color, front, nelem, moved, abandoned), the state after that layer.
    state: a seed_seq() result to start from (default: the seed of the inputs)."""
    tl, al = np.asarray(tetv).tolist(), np.asarray(adja).tolist()
    wl = np.asarray(w).tolist()
    star = [None] + stars(np.asarray(tetv)) + [[] for _ in range(np_)]
    st = state if state is not None else seed_seq(tetv, mark, w, np_)
    tmp, s, flag, bf = list(st["tmp"]), list(st["s"]), list(st["flag"]), st["bf"]
    mk = np.asarray(mark).tolist()
    negrp, nmin = np.asarray(nelem).tolist(), np.asarray(nemin).tolist()
    out = []
    for layer in range(nlayers):
        before = list(mk)
        abandoned = 0
        if set_pt is not None:
            for i, p in enumerate(np.asarray(set_pt).tolist()):
                if layer == 0 and set_color is not None:
                    tmp[p] = int(set_color[i])
                flag[p] = bf
        for p in range(1, np_ + 1):
            if flag[p] != bf and flag[p] != bf + 1:
                continue
            if not s[p]:
                continue  # (a point of no used tetra: the reference skips !MG_VOK)
            color = tmp[p]
            for n, k in enumerate(_ball(tl, al, star[p], p, s[p] // 4 - 1, ball)):
                if wl[mk[k]] <= wl[color]:
                    continue
                g = mk[k]
                if negrp[g] >= 0:
                    if (negrp[g] <= nmin[g]) if n == 0 else (negrp[g] == nmin[g]):
                        abandoned += 1
                        break
                    negrp[g] -= 1
                mk[k] = color
                j1 = tl[k].index(p)
                for j in range(1, 4):
                    j2 = (j1 + j) % 4
                    q = tl[k][j2]
                    if flag[q] != bf and flag[q] != bf + 1:
                        if wl[tmp[q]] > wl[color]:
                            tmp[q], s[q] = color, 4 * (k + 1) + j2
                        flag[q] = bf + 2
                    else:
                        flag[q] = bf + 1
        for p in range(1, np_ + 1):
            if flag[p] != bf + 1:
                continue
            lst = _ball(tl, al, star[p], p, s[p] // 4 - 1, ball)
            if side_tie == "bfs":
                for k in lst:
                    if wl[tmp[p]] > wl[mk[k]]:
                        tmp[p], s[p] = mk[k], 4 * (k + 1) + tl[k].index(p)
            else:
                best = min(lst, key=lambda k: (wl[mk[k]], k))
                if wl[tmp[p]] > wl[mk[best]]:
                    tmp[p], s[p] = mk[best], 4 * (best + 1) + tl[best].index(p)
            flag[p] += 1
        bf += 2
        out.append(dict(mark=np.array(mk, np.int32), color=np.array(tmp[1:], np.int32),
                        front=np.array([f == bf for f in flag[1:]], np.uint8), nelem=np.array(negrp, np.int32),
                        moved=sum(a != b for a, b in zip(before, mk)), abandoned=abandoned,
                        state=dict(tmp=list(tmp), s=list(s), flag=list(flag), bf=bf)))
    return out


# ---------------------------------------------------------------- the definition, in array operations

def seed_par(tetv, mark, w, np_):
    """(color [np], front [np] uint8)"""
    tetv, mark, w = np.asarray(tetv), np.asarray(mark), np.asarray(w, np.int64)
    used = tetv[:, 0] > 0
    k, c = np.nonzero(used[:, None] & np.ones(4, bool))
    corner = 4 * k + c
    p = tetv[k, c] - 1
    wc = w[mark[k]]
    big = np.iinfo(np.int64).max
    first = np.full(np_, big)
    np.minimum.at(first, p, corner)
    best = np.full(np_, big)
    np.minimum.at(best, p, (wc << 32) | corner)
    has = first != big
    color = np.full(np_, -1, np.int32)
    color[has] = mark[(best[has] & 0xFFFFFFFF) // 4]
    front = np.zeros(np_, np.uint8)
    front[has] = w[mark[first[has] // 4]] != (best[has] >> 32)
    return color, front


def layer_par(tetv, mark, w, nelem, nemin, color, front):
    """one layer from (mark, color, front), front including the caller's set points: dict(mark, color, front, D,
    moved, blocked); blocked: the inputs are returned unchanged"""
    tetv, w = np.asarray(tetv), np.asarray(w, np.int64)
    ne, ncolor = tetv.shape[0], w.size
    used = tetv[:, 0] > 0
    vs = np.sort(np.where(used[:, None], tetv, 1), axis=1) - 1  # a tetra's points in ascending id
    isf = front[vs].astype(bool) & used[:, None]
    cur = np.array(mark, np.int64)
    nev = np.zeros(ne, np.int64)
    last = np.zeros(ne, np.int64)
    D = np.zeros(ncolor, np.int64)
    for j in range(4):
        c = np.where(isf[:, j], color[vs[:, j]], 0)
        ev = isf[:, j] & (w[c] < w[cur])
        D += np.bincount(cur[ev], minlength=ncolor)
        cur = np.where(ev, c, cur)
        nev += ev
        last = np.where(ev, vs[:, j], last)
    nelem = np.asarray(nelem, np.int64)
    local = nelem >= 0
    if (local & (D > 0) & (D > nelem - np.asarray(nemin))).any():
        return dict(mark=np.array(mark, np.int32), color=color, front=front, D=D, moved=0, blocked=True)
    hit = nev > 0
    big = np.iinfo(np.int64).max
    # points off the front in a tetra with an event: the event of least (weight, point)
    key = np.full(color.size, big)
    side = np.zeros(color.size, bool)
    for j in range(4):
        q = vs[:, j]
        off = hit & ~isf[:, j]
        np.minimum.at(key, q[off], ((w[cur] << 32) | last)[off])
        side[q[hit & isf[:, j] & ((nev > 1) | (q != last))]] = True
    newc = color.copy()
    got = key != big
    wq = np.where(color >= 0, w[np.maximum(color, 0)], big)
    take = got & ((key >> 32) < wq)
    newc[take] = color[key[take] & 0xFFFFFFFF]
    # side points: the lowest tetra of least new weight over the star
    skey = np.full(color.size, big)
    tk = (w[cur] << 32) | np.arange(ne)
    for j in range(4):
        sel = used & side[vs[:, j]]
        np.minimum.at(skey, vs[sel, j], tk[sel])
    take = side & ((skey >> 32) < wq)
    newc[take] = cur[skey[take] & 0xFFFFFFFF]
    return dict(mark=cur.astype(np.int32), color=newc.astype(np.int32), front=(got | side).astype(np.uint8), D=D,
                moved=int(hit.sum()), blocked=False)


def ifc_par(tetv, mark, w, nelem, nemin, np_, nlayers, set_pt=None, set_color=None, color=None, front=None):
    """dict(layers = list of one dict per layer done (mark, color, front, nelem, moved), layers_done, blocked)"""
    if color is None:
        color, front = seed_par(tetv, mark, w, np_)
    color, front = np.array(color, np.int32), np.array(front, np.uint8)
    mark, nelem = np.array(mark, np.int32), np.array(nelem, np.int32)
    out = []
    for layer in range(nlayers):
        if set_pt is not None:
            sp = np.asarray(set_pt) - 1
            color, front = color.copy(), front.copy()  # (the previous layer's record keeps its arrays)
            if layer == 0 and set_color is not None:
                color[sp] = set_color
            front[sp] = 1
        r = layer_par(tetv, mark, w, nelem, nemin, color, front)
        if r["blocked"]:
            return dict(layers=out, layers_done=layer, blocked=1, color=color, front=front)
        mark, color, front = r["mark"], r["color"], r["front"]
        nelem = np.where(nelem >= 0, nelem - r["D"], nelem).astype(np.int32)
        out.append(dict(mark=mark, color=color, front=front, nelem=nelem, moved=r["moved"]))
    return dict(layers=out, layers_done=nlayers, blocked=0, color=color, front=front)


def remap(tetv, mark, ncolor, order):
    """(part, ngrp): the colours present among the used tetra numbered in ascending order[colour]; an unused
    tetra keeps 0"""
    tetv, mark, order = np.asarray(tetv), np.asarray(mark), np.asarray(order)
    used = tetv[:, 0] > 0
    present = np.zeros(ncolor, bool)
    present[mark[used]] = True
    new = np.zeros(ncolor, np.int32)
    cols = np.nonzero(present)[0]
    cols = cols[np.argsort(order[cols], kind="stable")]
    new[cols] = np.arange(cols.size)
    return np.where(used, new[np.where(used, mark, 0)], 0).astype(np.int32), int(cols.size)


# ---------------------------------------------------------------- fixtures

def weight_table(kind, mark, ncolor):
    """perm: all distinct; counts: the real tetra counts; ties: pairs of colours of equal weight"""
    if kind == "perm":
        return (np.random.default_rng(5).permutation(ncolor) + 1).astype(np.int32)
    if kind == "counts":
        return np.maximum(np.bincount(np.asarray(mark), minlength=ncolor), 1).astype(np.int32)
    if kind == "ties":
        return (5 + np.arange(ncolor) // 2).astype(np.int32)
    raise ValueError(kind)


WEIGHTS = ["perm", "counts", "ties"]


def path_mesh(ne):
    """a path of ne tetra: tetra k has the points k + 1 .. k + 4 and shares a face with k - 1 and k + 1.
    (tetv, adja, np)"""
    k = np.arange(ne)
    tetv = (k[:, None] + np.arange(1, 5)[None, :]).astype(np.int32)
    adja = np.zeros((ne, 4), np.int32)
    adja[1:, 3] = 4 * k[1:] + 0  # the face opposite the last point is shared with k - 1 (1-based id k), its face 0
    adja[:-1, 0] = 4 * (k[:-1] + 2) + 3
    return tetv, adja, ne + 3


def bands(ne, width, ncolor):
    return ((np.arange(ne) // width) % ncolor).astype(np.int32)
